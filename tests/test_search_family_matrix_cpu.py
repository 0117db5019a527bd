"""The waterfall-and-series family's launch-table model (tests/search_family_matrix.py) against the nine libraries' gfx950
code objects, both ways: every instantiation a library holds is named by a case of the model, and every case names an
instantiation a library holds.  So a table entry cannot land without a case that tests/test_search_family_matrix_gpu.py
launches, and a model that drifts from the tables fails here, without a GPU.  Kernel names only are read.  The rules the
model restates are held to each library's own geometry call where that reports the deciding value, at every case and on
both sides of every border."""
import importlib
import re

import numpy as np

import cand_ref
import clean_ref
import dedisp_form_cases as forms1
import ffa_ref
import fold_ref
import pulse_ref
import search_family_matrix as fm
import subdedisp_form_cases as forms2

IN_THE_PACKAGE = ("dedisp", "pulse", "fold")                 # bound by rtlws itself; the other six by a submodule each


def _module(built, lib):
    return built if lib in IN_THE_PACKAGE else importlib.import_module("rtlws." + lib)


def _path(built, lib):
    mod = _module(built, lib)
    (getattr(mod, lib + "_lib") if lib in IN_THE_PACKAGE else mod.lib)()
    return getattr(mod, lib.upper() + "_LIB")


def _arg(s):
    s = s.strip()
    return s == "true" if s in ("true", "false") else int(s) if re.fullmatch(r"-?\d+", s) else s.rsplit("::", 1)[-1]


def _library_kernels(built, lib):
    """The instantiations of librtlws_<lib>.so as (name, args); a kernel that is no template has no args."""
    from rtlws import codeobj
    found = set()
    for k in codeobj.kernels(_path(built, lib)):
        d = k.get("demangled", k["name"])
        m = re.match(r"^(?:void )?rtlws::%s::(\w+)(?:<([^>]*)>)?\(" % lib, d)
        assert m, d
        assert m.group(1) in fm.KERNELS[lib], d
        t = (m.group(1), tuple(_arg(a) for a in m.group(2).split(",")) if m.group(2) is not None else ())
        assert t not in found, d
        found.add(t)
    return found


def test_every_instantiation_has_a_case_and_every_case_an_instantiation(built):
    held = {lib: _library_kernels(built, lib) for lib in fm.LIBRARIES}
    modelled = {}
    for c in fm.CASES:
        modelled.setdefault((c.lib, fm.instantiation(c)), []).append(c)
    everything = {(lib, t) for lib in fm.LIBRARIES for t in held[lib]}
    untested = sorted(everything - set(modelled), key=str)
    phantom = sorted(((t, [c.label() for c in modelled[t]]) for t in set(modelled) - everything), key=str)
    assert not untested, "instantiations no case reaches: %s" % [fm.spell(t[1]) for t in untested]
    assert not phantom, "cases that name no instantiation: %s" % phantom
    counts = {lib: len(held[lib]) for lib in fm.LIBRARIES}
    print("%d search-family instantiations, matched by %d cases (%d of them for a geometry class): %s"
          % (len(everything), len(fm.CASES), len(fm.CLASS_CASES), counts))
    assert counts == fm.COUNTS == {"dedisp": 9, "subdedisp": 16, "pulse": 5, "fold": 3, "ffa": 3, "cdd": 6, "cand": 11, "clean": 7, "sift": 3}
    assert len(everything) == 63
    # an instantiation's own cases: one, or one per form it chooses among at run time
    own = {}
    for c in fm.INSTANTIATION_CASES:
        own.setdefault((c.lib, fm.instantiation(c)), []).append(c.form)
    assert set(own) == everything
    forms_of = {"fold_kernel": ["hits", "no hits"], "cand_fold_kernel": ["hits", "no hits"], "cdd_kernel": ["voltages", "time", "channel"],
                "clean_apply_kernel": ["zero-DM", "no zero-DM"]}
    for (lib, t), forms in own.items():
        want = forms_of.get(t[0], [""])
        if t[0] == "cand_stage_kernel":
            want = ["stage 2"] if t[1][1] else ["stage 1, copy", "stage 1, no copy"]
        elif t == ("ffa_pass", (True,)):
            want = ["the last of 1", "the last of 2", "the last of 3"]
        elif t == ("ffa_pass", (False,)):
            want = ["not the last pass"]
        assert forms == want, (fm.spell(t), forms)
    assert len(fm.INSTANTIATION_CASES) == 63 + 3 + 3 + 2 + 12 + 4 + 5 == 92 and sum(f == "voltages" or f in ("time", "channel") for fs in own.values() for f in fs) == 18
    assert len({c.label() for c in fm.CASES}) == len(fm.CASES)


def test_the_form_files_cases_are_taken_not_restated():
    """the two dedispersions' cases are members of the form files' lists, each the first whose plan is the instantiation"""
    for c in fm.by_library("dedisp"):
        assert c.plan in forms1.CASES
        mine = [k for k in forms1.CASES if fm.instantiation(c._replace(plan=k)) == fm.instantiation(c)]
        assert mine[0] is c.plan or mine[0] == c.plan
    for c in fm.by_library("subdedisp"):
        pool = forms2.STAGE1_CASES if c.kernel == "subdedisp_subband_kernel" else forms2.STAGE2_CASES
        assert c.plan in pool and [k for k in pool if fm.instantiation(c._replace(plan=k)) == fm.instantiation(c)][0] == c.plan
    # the tables: every trial count in either LDS, one lone form; stage 2 without a second LDS at one trial
    assert sorted(fm.instantiation(c)[1] for c in fm.by_library("dedisp")) == sorted([(t, False, b) for t in (1, 2, 4, 8) for b in (False, True)] + [(1, True, False)])
    two = sorted(fm.instantiation(c)[1] for c in fm.by_library("subdedisp") if c.kernel == "subdedisp_trial_kernel")
    assert two == sorted([(t, b) for t in (2, 4, 8) for b in (False, True)] + [(1, False)])


def test_the_dedispersions_rules_against_their_geometry(built):
    """the LDS bytes and the trials a workgroup that rtlws_dedisp_geometry and rtlws_subdedisp_geometry report for the
    cases' tables are the form the model turns into template arguments; on both sides of every border of
    tests/dedisp_form_cases.py and subdedisp_form_cases.py the arguments change as the tables say"""
    import rtlws.subdedisp as sd
    for c in fm.by_library("dedisp"):
        rc, _, threads, lds, tile, per, _ = built.dedisp_geometry(forms1.table(c.plan), None, forms1.NOUT)
        form = forms1.form(c.plan.plan_spread, c.plan.plan_per)
        assert (rc, threads, tile, per, lds) == (0, 256, forms1.TILE, c.plan.plan_per, form[1]), c.label()
        assert fm.instantiation(c)[1] == ((1, True, False) if form[0] == "lone" else (per, False, lds == 65536))
    for c in fm.by_library("subdedisp"):
        first, d1, d2 = (forms2.stage1_case_tables if c.kernel == "subdedisp_subband_kernel" else forms2.stage2_case_tables)(c.plan)
        got = sd.geometry(first, d1, d2, None, forms2.NOUT)
        stage = 0 if c.kernel == "subdedisp_subband_kernel" else 1
        assert got[0] == 0 and got[5 + stage] == c.plan.plan_per, c.label()
        args = fm.instantiation(c)[1]
        assert (args[0], args[-1]) == (got[5 + stage], got[3][stage] == 65536), c.label()
    for (chunk, lds), last, beyond in forms1.BORDERS:
        for per in ((1,) if chunk != 32 else fm.TRIAL_COUNTS):
            assert fm.dedisp_args(forms1.form(last, per), per) == ((1, True, False) if chunk == "lone" else (per, False, lds == 65536))
            after = forms1.form(beyond, per) if beyond is not None else None
            assert after is None or fm.dedisp_args(after, per) != fm.dedisp_args(forms1.form(last, per), per)
    assert forms1.form(248, 8) is None and forms1.form(3777, 1)[0] == "lone"
    for lds, last, beyond in forms2.BORDERS2:
        for per in fm.STAGE2_GROUPS:
            assert fm.stage2_args(forms2.form2(last, per), per) == (per, lds == 65536)
        assert forms2.form2(beyond, 8) is None or fm.stage2_args(forms2.form2(beyond, 8), 8) == (8, True)
    assert fm.stage2_args(forms2.form2(0, 1), 1) == (1, False)


def test_the_pulse_rule_against_its_geometry(built):
    """the tile and the LDS bytes rtlws_pulse_geometry reports are pulse_kernel's <WORDS, U>: at every case, at every width
    1 .. 1024 alone (every border of one width's plan lies between two of them) and on both sides of the first table
    beside 1024 that takes each tile"""
    def check(widths):
        rc, _, threads, lds, tile, _, _ = built.pulse_geometry(widths, 64)
        assert rc == 0 and threads == fm.PULSE_THREADS and fm.pulse_args(widths) == (lds // 4, tile // 256), widths
        return fm.pulse_args(widths)
    cases = fm.by_library("pulse")
    assert [check(c.plan) for c in cases] == [fm.instantiation(c)[1] for c in cases] == [(4096, 4), (8192, 4), (16384, 4), (16384, 2), (16384, 1)]
    alone = [check((w,)) for w in range(1, 1025)]
    beside = [check((w, 1024)) for w in range(1, 1024)]
    for c in cases:
        args, w = fm.instantiation(c)[1], c.plan[0]
        # the smallest: the table before it (one width less, or the last single width) takes another instantiation
        seen = alone[:w - 1] if len(c.plan) == 1 else alone + beside[:w - 1]
        assert args not in seen and (alone[w - 1] if len(c.plan) == 1 else beside[w - 1]) == args, c.label()
    print("pulse: the smallest tables " + ", ".join("%s %s" % (fm.spell(fm.instantiation(c)), c.plan) for c in cases))


def test_the_folds_rules_against_their_geometry(built):
    """waves_per_block as rtlws_fold_geometry and rtlws_cand_fold_geometry report it, at every case and on both sides of 64
    and 128 bins; the refinement's LDS and threads (per_lane itself is not reported: its borders are held to ceil(nbins / 64))"""
    import rtlws.cand as cand
    for nbins in sorted({c.plan[0] for c in fm.CASES if c.kernel in ("fold_kernel", "cand_fold_kernel")} | {2, 64, 65, 128, 129, 256}):
        wpb = fold_ref.waves_per_block(nbins)
        assert wpb == cand_ref.waves_per_block(nbins) == (4 if nbins <= 64 else 2 if nbins <= 128 else 1)
        rc, _, threads, lds, _, got, _ = built.fold_geometry(1, nbins, 64)
        assert (rc, threads, lds, got) == (0, 64 * wpb, wpb * nbins * 256, wpb), nbins
        rc, _, threads, lds, got, _ = cand.fold_geometry(1, 4, nbins, 16)
        assert (rc, threads, lds, got) == (0, 64 * wpb, wpb * nbins * 256, wpb), nbins
    assert [fm.instantiation(c)[1][0] for c in fm.by_library("fold")] == [4, 4, 2, 2, 1, 1]
    for c in fm.CASES:
        if c.kernel == "cand_stage_kernel":
            nbins, nsub, ndm, ntr, nchan = c.plan
            assert cand.search_geometry(1, nsub, nchan, nbins, ndm, ntr) == (0,) + cand_ref.search_plan(1, nsub, nchan, nbins, ndm, ntr), c.label()
    assert [fm.per_lane(n) for n in (2, 64, 65, 128, 129, 192, 193, 256)] == [1, 1, 2, 2, 3, 3, 4, 4]
    nsub, ndm, ntr, nchan = fm.SEARCH_BORDERS
    assert min(nsub, nchan) > cand_ref.CHUNK and min(ndm, ntr) > cand_ref.WAVES                  # both stages cross both tiles
    nsub, ndm, ntr, nchan = fm.SEARCH_SMALL
    assert max(nsub, nchan) <= cand_ref.CHUNK and max(ndm, ntr) <= cand_ref.WAVES


def test_the_ffa_rule_against_its_geometry(built):
    """the passes, their stages and the merge as rtlws_ffa_geometry reports them, at every case and on both sides of the
    pitches at which a pass takes one stage fewer; the cases are the fewest cells of their pass count"""
    import rtlws.ffa as ffa
    for c in fm.by_library("ffa"):
        p0, L, seg = c.plan
        rc, passes, stages, _, _, _, merge, _, _ = ffa.geometry(p0, 1, L, fm.FFA_WIDTHS, seg)
        launches = fm.ffa_launches(p0, 1, L, seg)
        assert rc == 0 and list(stages[:passes]) == ffa_ref.split(L, p0) and sum(stages) == L
        assert [t for t in launches if t[0] == "ffa_pass"] == [("ffa_pass", (False,))] * (passes - 1) + [("ffa_pass", (True,))]
        assert (("ffa_merge", ()) in launches) == bool(merge) == (seg > 1 << stages[passes - 1]), c.label()
        assert fm.instantiation(c) in launches
    plans = [c.plan for c in fm.by_library("ffa")]
    assert plans == [(16, 1, 1), (16, 8, 1), (625, 9, 1), (16, 8, 2), (16, 8, 256)]
    borders = [p for p in range(ffa_ref.MIN_P, ffa_ref.MAX_P) if ffa_ref.max_stages(p) != ffa_ref.max_stages(p + 1)]
    # (4 << n) pitch 4 + (128 << n) <= 160 KiB: seven stages up to a pitch of 144, six up to 304, five up to 624, then four
    assert borders == [144, 304, 624] and [ffa_ref.max_stages(p) for p in borders + [625]] == [7, 6, 5, 4]
    for p in borders:
        for pitch in (p, p + 1):
            most = ffa_ref.max_stages(pitch)
            for L in (most, most + 1, 2 * most, 2 * most + 1):
                if L <= ffa_ref.MAX_L and (pitch << L) <= ffa_ref.MAX_CELLS:
                    rc, passes, stages, _, _, _, merge, _, _ = ffa.geometry(pitch, 1, L, fm.FFA_WIDTHS, 1 << L)
                    assert rc == 0 and passes == -(-L // most) == len(fm.ffa_launches(pitch, 1, L, 1)), (pitch, L)
                    assert bool(merge) == (("ffa_merge", ()) in fm.ffa_launches(pitch, 1, L, 1 << L)) == (passes > 1), (pitch, L)


def test_the_cdd_rule_against_its_geometry(built):
    import rtlws.cdd as cdd
    for log2n in fm.LOG2NS:
        for ksum in (0, 3):
            lead, trail = (5, 12) if log2n % 2 else (5, 11)
            assert cdd.geometry(log2n, lead, trail, 2, ksum, 2) == (0, 4, fm.cdd_threads(log2n), fm.cdd_lds(log2n))
    assert cdd.geometry(8, 5, 11, 2)[0] != 0 and cdd.geometry(15, 5, 11, 2)[0] != 0
    assert [fm.cdd_threads(k) for k in fm.LOG2NS] == [64, 64, 128, 256, 512, 1024] and fm.cdd_lds(14) == 136 * 1024


def test_the_clean_rules_against_its_geometry(built):
    """every channel count 4 .. 4096 -- every case and both sides of every border among them: what rtlws_clean_geometry
    reports of the three launches is the model's row_threads, row_waves, sort_len, flag_threads and LDS bytes"""
    import rtlws.clean as clean
    B = 16384                                                  # one block; its rows over 16 T / G a workgroup: G from the grid
    seen = set()
    for m in range(4, 4097, 4):
        rc, blocks, threads, lds, nblocks, _, _ = clean.geometry(m, B, B)
        assert rc == 0 and nblocks == 1
        assert tuple(threads) == (512, fm.flag_threads(m), fm.apply_threads(m)) and tuple(lds) == (32768, fm.flag_lds(m), fm.apply_lds(m)), m
        assert blocks[2] * threads[2] == 1024 * fm.row_threads(m) and blocks[0] == -(-m // 256) and blocks[1] == 1, m
        assert (clean.geometry(m, 32, 80)[1:4], clean.geometry(m, 32, 80)[4]) == (clean_ref.geometry(m, 32, 80)[:3], 3), m
        assert fm.sort_len(m) == (lds[1] - 128) // 16 and fm.per_thread(m) * threads[1] >= fm.sort_len(m) > (fm.per_thread(m) - 1) * threads[1]
        seen.add((fm.row_threads(m), fm.row_waves(m), fm.sort_len(m), threads[1], fm.per_thread(m), lds[1] > 65536))
    assert {s[1] for s in seen} == set(fm.ROW_WAVES) and {s[0] for s in seen} == {1 << k for k in range(11)}
    assert [fm.row_waves(m) for m in (256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096)] == [1, 2, 2, 4, 4, 8, 8, 16, 16]
    assert [fm.flag_lds(m) for m in fm.FLAG_LDS_BORDER] == [32896, 65664]
    assert {(s[3], s[4]) for s in seen} == {(64, 1), (64, 2), (128, 2), (256, 2), (512, 2), (1024, 2), (1024, 4)}
    assert {s[2] for s in seen if s[3:5] == (64, 2)} == {128} and {s[2] for s in seen if s[3:5] == (1024, 2)} == {2048}


def test_every_class_has_a_case():
    """every row_threads 1 .. 1024 at an exact and at a padded channel count where both exist, every sort_len, every
    (flag_threads, keys a thread) pair, both sides of flag_lds > 65536; per_lane on both sides of its three borders"""
    reached = {cl for c in fm.CASES for cl in fm.classes(c)}
    assert reached == set(fm.ALL_CLASSES), sorted(set(fm.ALL_CLASSES) - reached, key=str)
    assert {cl for c in fm.CLASS_CASES for cl in fm.classes(c)} == reached                          # ... by the class cases alone
    lanes = {(cl[1], cl[2]) for cl in reached if cl[0] == "row_threads"}
    assert lanes == {(1 << k, "exact") for k in range(11)} | {(1 << k, "padded") for k in range(2, 11)}
    assert {cl[1] for cl in reached if cl[0] == "sort_len"} == {4 << k for k in range(11)}
    assert {cl[1:] for cl in reached if cl[0] == "flag_lds > 65536"} == {(False, 2048), (True, 2052)}
    assert {cl[1:] for cl in reached if cl[0] == "per_lane"} == {(1, 64), (2, 65), (2, 128), (3, 129), (3, 192), (4, 193)}
    assert [c.plan[0] for c in fm.CLASS_CASES if c.lib == "clean"] == [4, 8, 12, 16, 20, 32, 36, 64, 68, 128, 132, 256, 260, 512, 516, 1024, 1028, 2048, 2052, 4096]
    assert all(fm.instantiation(c)[1] == (fm.row_waves(c.plan[0]),) for c in fm.CLASS_CASES if c.lib == "clean")


def _launched_before():
    """-> (the instantiations, the classes) that a comparison of the earlier suites reaches, from their own
    parametrisations (imported where they are data, restated where a test fixes its shape in its body)."""
    import test_cand_gpu as cand
    import test_clean_gpu as clean
    import test_fold_gpu as fold
    import test_pulse_gpu as pulse

    seen, classes = set(), set()
    # both dedispersions: every case of the form files (test_every_border_of_the_plan, _of_stage_1, _of_stage_2)
    seen.update(("dedisp_kernel", fm.dedisp_args(forms1.form(c.plan_spread, c.plan_per), c.plan_per)) for c in forms1.CASES)
    seen.update(("subdedisp_subband_kernel", fm.dedisp_args(forms1.form(c.plan_spread, c.plan_per), c.plan_per)) for c in forms2.STAGE1_CASES)
    seen.update(("subdedisp_trial_kernel", fm.stage2_args(forms2.form2(c.plan_spread, c.plan_per), c.plan_per)) for c in forms2.STAGE2_CASES)
    # the pulse search: test_every_plan_at_every_border's tables before this matrix, and the tables its other tests, the
    # sift's and the chains fix
    others = [(1, 3, 8, 100), (1, 2, 3, 8, 100), (1, 3, 8), (3, 258), pulse.CHAIN_WIDTHS, (1, 2, 4, 8, 16), (1, 3, 4), (1, 2, 4, 8), (1,)]
    seen.update(("pulse_kernel", fm.pulse_args(w)) for w in list(pulse.FIRST_PLANS.values()) + others)
    seen.update(("fold_kernel", (fold_ref.waves_per_block(n), "RowReads")) for n in fold.NBINS)   # test_every_block_shape_at_every_border
    seen.update(("cand_fold_kernel", (cand_ref.waves_per_block(n),)) for n in cand.NBINS)         # test_every_block_shape_and_lane_group_count
    # the refinement: the bin counts of test_every_count_of_bins_per_lane_and_every_tile_border before this matrix, and
    # 129 (the outputs on and off, one plan many times), 50 (special values, many times) and 65 (the captured graph)
    bins = set(cand.FIRST_SEARCH_BINS) | {129, 50, 65}
    seen.update(("cand_stage_kernel", (fm.per_lane(n), sums)) for n in bins for sums in (False, True))
    classes.update(cl for n in bins for cl in fm.cand_classes(n))
    # the fast folding: test_every_pass_count's three plans at p0 1024 and test_segments_on_both_sides_of_the_merge's at 700
    for p0, L, seg in [(1024, L, 1) for L in range(1, 10)] + [(700, 6, 64)]:
        seen.update(fm.ffa_launches(p0, 1, L, seg))
    seen.update(("cdd_kernel", (k,)) for k in range(9, 15))                                        # test_voltages_within_both_bounds
    # the cleaning: the feature's own channel counts; its other tests' shapes are among them
    assert {12, 260, 1024, 4096, 4, 252, 64} <= set(clean.FIRST_NCHANS)
    seen.update({("clean_stats_kernel", ()), ("clean_flags_kernel", ())})
    seen.update(("clean_apply_kernel", (fm.row_waves(m),)) for m in clean.FIRST_NCHANS)
    classes.update(cl for m in clean.FIRST_NCHANS for cl in fm.clean_classes(m))
    seen.update((k, ()) for k in fm.KERNELS["sift"])                                               # every run launches the three
    return seen, classes


def test_first_launched_here_is_what_no_earlier_suite_reached():
    """The pinned list is a part of the matrix, holds clean_apply_kernel<8>, and is exactly what is left of the family's
    63 instantiations and of the classes when those that the earlier suites' parametrisations reach are taken away."""
    matrix = {fm.instantiation(c) for c in fm.CASES}
    first = set(fm.FIRST_LAUNCHED_HERE)
    assert len(first) == len(fm.FIRST_LAUNCHED_HERE) == 25 and ("clean_apply_kernel", (8,)) in first
    before, classes_before = _launched_before()
    assert before <= matrix and len(matrix) == 63 and classes_before <= set(fm.ALL_CLASSES)
    left = (matrix - before) | (set(fm.ALL_CLASSES) - classes_before)
    assert left == first, (sorted(left - first, key=str), sorted(first - left, key=str))
    assert matrix - before == {("clean_apply_kernel", (8,)), ("pulse_kernel", (16384, 4))}
    print("first launched by the matrix: %s; and the classes %s"
          % (", ".join(fm.spell(t) for t in fm.FIRST_LAUNCHED_HERE if t in matrix), ", ".join(" ".join(str(v) for v in t) for t in fm.FIRST_LAUNCHED_HERE if t not in matrix)))


def test_the_extended_suites_reach_what_the_matrix_found():
    """the lists of tests/test_clean_gpu.py and tests/test_cand_gpu.py as they stand now take every class themselves"""
    import test_cand_gpu as cand
    import test_cdd_gpu as cdd
    import test_clean_gpu as clean
    assert set(clean.NCHANS) == set(clean.FIRST_NCHANS) | {8, 20, 128, 516, 1028, 2048, 2052}
    got = {cl[:2] for m in clean.NCHANS for cl in fm.clean_classes(m)}
    assert {cl[:2] for cl in fm.ALL_CLASSES if cl[0] != "per_lane"} <= got | {("flag_lds > 65536", False), ("flag_lds > 65536", True)}
    assert {fm.row_waves(m) for m in clean.NCHANS} == set(fm.ROW_WAVES)
    assert {n for n, nchan in cand.SEARCH_BINS if nchan == 68} >= set(fm.PER_LANE_BORDERS)
    import test_pulse_gpu as pulse
    assert {fm.pulse_args(w) for w in pulse.PLANS.values()} == {fm.instantiation(c)[1] for c in fm.by_library("pulse")}
    assert {(k, lay) for k, which, lay in cdd.POWER_CASES if which == "3"} == {(k, lay) for k in fm.LOG2NS for lay in ("time", "channel")}
    assert np.all(np.diff(clean.NCHANS) > 0)

"""A model of the waterfall-and-series family's launch tables: which kernel instantiation a plan and a run launch.

Restated from rtl-ws_amd/csrc (no GPU, no build needed), the nine libraries behind search_plan.h:
  dedisp.hip ...... with_kernel:   dedisp_kernel<TRIALS, LONE, BIG>, TRIALS 8, 4, 2, 1; LONE only as <1, true, false>
  subdedisp.hip ... with_stage1:   subdedisp_subband_kernel<TRIALS, LONE, BIG>, the same nine
                    with_stage2:   subdedisp_trial_kernel<TRIALS, BIG>, TRIALS 8, 4, 2 in either LDS and <1, false>
  pulse.hip ....... with_kernel:   pulse_kernel<WORDS, U>: a tile of 1024 (U 4) in 16, 32 or 64 KiB, of 512 and 256 in 64 KiB
  fold.hip ........ with_kernel:   fold_kernel<WPB, RowReads>, WPB 4, 2, 1                    (hits or none: a branch at run time)
  cand.hip ........ with_fold_kernel: cand_fold_kernel<WPB>                                   (the same branch)
                    launch_stage:  cand_stage_kernel<R, SUMS>, R = ceil(nbins / 64) = 1 .. 4   (copy or none: a branch)
  ffa.hip ......... launch_pass:   ffa_pass<LAST>; launch_merge: ffa_merge                     (one to three passes a plan)
  cdd.hip ......... launch:        cdd_kernel<LOG2N>, 9 .. 14                      (voltages and both layouts of the power rows: branches)
  clean.hip ....... clean_stats_kernel, clean_flags_kernel, clean_apply_kernel<W>, W = row_waves 1, 2, 4, 8, 16 (zero-DM: a branch)
  sift.hip ........ sift_score_kernel, sift_box_kernel, sift_list_kernel: every run launches all three

63 instantiations.  A rule that a suite's restatement already words (tests/dedisp_form_cases.py, subdedisp_form_cases.py,
pulse_ref.py, fold_ref.py, cand_ref.py, ffa_ref.py, clean_ref.py) is taken from there; the table that turns its value into
template arguments is worded here.

INSTANTIATION_CASES holds one case per instantiation and, for a kernel that chooses among forms at run time, one per form;
each names the smallest plan that reaches it (for the two dedispersions: the first case of the form files that does).
CLASS_CASES holds the geometry classes of the cleaning (every row_threads 1 .. 1024 at an exact and a padded channel count,
which between them take every sort_len 4 .. 4096, every (flag_threads, channels a thread) pair and both sides of
flag_lds > 65536) and the refinement's per_lane(nbins) on both sides of each of its borders.  CASES is both.
tests/test_search_family_matrix_cpu.py holds the model to the nine libraries' code objects both ways and to their geometry
calls, tests/test_search_family_matrix_gpu.py launches every case through its suite's own checked path."""
from collections import namedtuple

import cand_ref
import clean_ref
import dedisp_form_cases as forms1
import ffa_ref
import fold_ref
import pulse_ref
import subdedisp_form_cases as forms2

LIBRARIES = ("dedisp", "subdedisp", "pulse", "fold", "ffa", "cdd", "cand", "clean", "sift")
# the kernels of each library, as its code object names them
KERNELS = {"dedisp": ("dedisp_kernel",), "subdedisp": ("subdedisp_subband_kernel", "subdedisp_trial_kernel"), "pulse": ("pulse_kernel",),
           "fold": ("fold_kernel",), "ffa": ("ffa_pass", "ffa_merge"), "cdd": ("cdd_kernel",),
           "cand": ("cand_fold_kernel", "cand_stage_kernel"), "clean": ("clean_stats_kernel", "clean_flags_kernel", "clean_apply_kernel"),
           "sift": ("sift_score_kernel", "sift_box_kernel", "sift_list_kernel")}
COUNTS = {"dedisp": 9, "subdedisp": 16, "pulse": 5, "fold": 3, "ffa": 3, "cdd": 6, "cand": 11, "clean": 7, "sift": 3}

# ---- the tables, as the .hip files word them -------------------------------------------------------------------------
TRIAL_COUNTS = (8, 4, 2, 1)                                   # dedisp.hip, subdedisp.hip: TrialCounts
STAGE2_GROUPS = (8, 4, 2)                                     # subdedisp.hip with_stage2: Vals<8, 4, 2>, and one trial beside them
PULSE_LDS_WORDS = (4096, 8192, 16384)                         # pulse.h: LDS_WORDS
PULSE_THREADS = 256                                           # pulse.h: THREADS; U = tile_out / THREADS
WAVES_PER_BLOCK = (4, 2, 1)                                   # fold.hip, cand.hip: the switch over waves_per_block
PER_LANE = (1, 2, 3, 4)                                       # cand.hip: PerLane
LOG2NS = tuple(range(9, 15))                                  # cdd.hip: Log2Ns
ROW_WAVES = (1, 2, 4, 8, 16)                                  # clean.hip: RowWaves
LANES = 64


def dedisp_args(form, per):
    """dedisp.hip with_kernel (and subdedisp.hip with_stage1) of dedisp_form_cases.form's (chunk or "lone", LDS bytes, stride)"""
    chunk, lds, _ = form
    if chunk == "lone":
        assert per == 1 and lds == forms1.SMALL_LDS
        return (1, True, False)
    assert per in TRIAL_COUNTS
    return (per, False, lds == forms1.BIG_LDS)


def stage2_args(form, per):
    """subdedisp.hip with_stage2 of subdedisp_form_cases.form2's (LDS bytes, stride)"""
    lds, _ = form
    if per == 1:
        assert lds == forms2.SMALL_LDS
        return (1, False)
    assert per in STAGE2_GROUPS
    return (per, lds == forms2.BIG_LDS)


def pulse_args(widths):
    """pulse.hip with_kernel of pulse_ref.plan's (tile_out, LDS bytes, ..): a tile below 1024 only in the largest LDS"""
    tile, lds = pulse_ref.plan(widths)[:2]
    assert lds // 4 in PULSE_LDS_WORDS and tile in (1024, 512, 256) and (tile == 1024 or lds // 4 == PULSE_LDS_WORDS[2])
    return (lds // 4, tile // PULSE_THREADS)


def per_lane(nbins):
    """cand.hip"""
    return -(-nbins // LANES)


def ffa_launches(p0, nper, L, seg):
    """ffa_shim.hip's run: every pass but the last is ffa_pass<false>, the last ffa_pass<true>, and ffa_merge follows where
    a segment holds more rows than a workgroup of the last pass"""
    stages = ffa_ref.split(L, p0 + nper - 1)
    return [("ffa_pass", (False,))] * (len(stages) - 1) + [("ffa_pass", (True,))] + ([("ffa_merge", ())] if seg > 1 << stages[-1] else [])


def cdd_threads(log2n):
    """cdd.h threads_of, lds_of"""
    return max(1 << (log2n - 4), LANES)


def cdd_lds(log2n):
    return 8 * ((1 << log2n) + (1 << (log2n - 4)))


# clean.h
def row_threads(nchan):
    return clean_ref.pow2_at_least(nchan // 4)


def row_waves(nchan):
    return 1 if row_threads(nchan) <= LANES else row_threads(nchan) // LANES


def apply_threads(nchan):
    return max(row_waves(nchan), 4) * LANES


def apply_lds(nchan):
    return 2 * apply_threads(nchan) * 4 if row_waves(nchan) > 1 else 0


def sort_len(nchan):
    return clean_ref.pow2_at_least(nchan)


def flag_threads(nchan):
    return min(max(sort_len(nchan) // 2, LANES), 1024)


def per_thread(nchan):
    """the keys a thread of stage 2 holds: its registers e with tid + e * threads < sort_len"""
    return -(-sort_len(nchan) // flag_threads(nchan))


def flag_lds(nchan):
    return 2 * sort_len(nchan) * 8 + 128


def clean_classes(nchan):
    """the classes a channel count falls into: the deciding values of stages 2 and 3"""
    G = row_threads(nchan)
    out = [("row_threads", G, "exact" if 4 * G == nchan else "padded"), ("sort_len", sort_len(nchan)), ("flag_threads x keys", flag_threads(nchan), per_thread(nchan))]
    if nchan in FLAG_LDS_BORDER:
        out.append(("flag_lds > 65536", flag_lds(nchan) > 65536, nchan))
    return out


FLAG_LDS_BORDER = (2048, 2052)                                # the last channel count under 64 KiB and the first above it
assert flag_lds(2048) <= 65536 < flag_lds(2052) and all(flag_lds(m) > 65536 for m in range(2052, 4097, 4)) and all(flag_lds(m) <= 65536 for m in range(4, 2049, 4))


# ---- the cases ----------------------------------------------------------------------------------------------------------
class Case(namedtuple("Case", "lib kernel form plan why")):
    """lib: one of LIBRARIES; kernel: the one of the plan's launches the case is there for; form: the branch it takes at
    run time ("" where it has none); plan: what opens it -- a case of the form files, a width table, (nbins,), (nbins, nsub,
    ndm, ntr, nchan), (p0, L, seg), (log2n,), (nchan,) or a name; why: "" for an instantiation's case, else its class"""

    def label(self):
        plan = self.plan
        if self.lib == "dedisp" or self.kernel == "subdedisp_subband_kernel":
            plan = forms1.case_id(plan)
        elif self.kernel == "subdedisp_trial_kernel":
            plan = forms2.case2_id(plan)
        elif not isinstance(plan, str):
            plan = "x".join(str(v) for v in plan)
        return " ".join(s for s in (self.kernel, self.form, plan, self.why and "(%s)" % self.why) if s)


SEARCH_SMALL = (3, 5, 7, 4)                                   # (nsub, ndm, ntr, nchan) of a refinement: one chunk, one group of trials
SEARCH_BORDERS = (33, 9, 9, 36)                               # both stages across the chunk of 32 rows and the 8 trials of a workgroup
FFA_WIDTHS = (1, 3)


def instantiation(c):
    """(kernel name, template arguments) of the instantiation case c is there for, by the rules above; the arguments as the
    demangled name spells them: clean_apply_kernel<8> -> ("clean_apply_kernel", (8,)), ffa_merge -> ("ffa_merge", ())"""
    assert c.lib in LIBRARIES and c.kernel in KERNELS[c.lib], c
    if c.kernel in ("dedisp_kernel", "subdedisp_subband_kernel"):
        return (c.kernel, dedisp_args(forms1.form(c.plan.plan_spread, c.plan.plan_per), c.plan.plan_per))
    if c.kernel == "subdedisp_trial_kernel":
        return (c.kernel, stage2_args(forms2.form2(c.plan.plan_spread, c.plan.plan_per), c.plan.plan_per))
    if c.kernel == "pulse_kernel":
        return (c.kernel, pulse_args(c.plan))
    if c.kernel == "fold_kernel":
        assert fold_ref.waves_per_block(c.plan[0]) in WAVES_PER_BLOCK
        return (c.kernel, (fold_ref.waves_per_block(c.plan[0]), "RowReads"))
    if c.kernel == "cand_fold_kernel":
        assert cand_ref.waves_per_block(c.plan[0]) in WAVES_PER_BLOCK
        return (c.kernel, (cand_ref.waves_per_block(c.plan[0]),))
    if c.kernel == "cand_stage_kernel":
        assert per_lane(c.plan[0]) in PER_LANE
        return (c.kernel, (per_lane(c.plan[0]), c.form == "stage 2"))
    if c.lib == "ffa":
        p0, L, seg = c.plan
        launches = ffa_launches(p0, 1, L, seg)
        mine = [t for t in launches if t[0] == c.kernel and (c.kernel == "ffa_merge" or t[1] == (c.form != "not the last pass",))]
        assert mine and (not c.form.startswith("the last of") or c.form == "the last of %d" % sum(t[0] == "ffa_pass" for t in launches)), c
        return mine[0]
    if c.kernel == "cdd_kernel":
        assert c.plan[0] in LOG2NS
        return (c.kernel, c.plan)
    if c.kernel == "clean_apply_kernel":
        assert row_waves(c.plan[0]) in ROW_WAVES
        return (c.kernel, (row_waves(c.plan[0]),))
    return (c.kernel, ())                                     # clean's first two launches and the sift's three: no instantiations


def _smallest_pulse_tables():
    """per (WORDS, U) the first table that takes it among one width 1 .. 1024 and then a width beside 1024"""
    found = {}
    for widths in [(w,) for w in range(1, 1025)] + [(w, 1024) for w in range(1, 1024)]:
        found.setdefault(pulse_args(widths), widths)
    return found


def _smallest_ffa_plan(passes):
    """(p0, L) of the fewest cells p0 2^L whose stages split into `passes` passes"""
    best = None
    for p0 in range(ffa_ref.MIN_P, ffa_ref.MAX_P + 1):
        for L in range(1, ffa_ref.MAX_L + 1):
            if ffa_ref.supported(p0, 1, L, FFA_WIDTHS, 1) and len(ffa_ref.split(L, p0)) == passes and (best is None or p0 << L < best[0] << best[1]):
                best = (p0, L)
    return best


def _instantiation_cases():
    out = []
    # the two dedispersions: the first case of the form files whose plan is the instantiation
    for per in TRIAL_COUNTS:
        for big in (False, True):
            want = (per, False, big)
            pick = lambda c: dedisp_args(forms1.form(c.plan_spread, c.plan_per), c.plan_per) == want
            out.append(Case("dedisp", "dedisp_kernel", "", next(c for c in forms1.CASES if pick(c)), ""))
            out.append(Case("subdedisp", "subdedisp_subband_kernel", "", next(c for c in forms2.STAGE1_CASES if pick(c)), ""))
    lone = lambda c: forms1.form(c.plan_spread, c.plan_per)[0] == "lone"
    out.append(Case("dedisp", "dedisp_kernel", "", next(c for c in forms1.CASES if lone(c)), ""))
    out.append(Case("subdedisp", "subdedisp_subband_kernel", "", next(c for c in forms2.STAGE1_CASES if lone(c)), ""))
    for want in [(per, big) for per in STAGE2_GROUPS for big in (False, True)] + [(1, False)]:
        pick = lambda c: stage2_args(forms2.form2(c.plan_spread, c.plan_per), c.plan_per) == want
        out.append(Case("subdedisp", "subdedisp_trial_kernel", "", next(c for c in forms2.STAGE2_CASES if pick(c)), ""))
    tables = _smallest_pulse_tables()
    for key in [(words, 4) for words in PULSE_LDS_WORDS] + [(PULSE_LDS_WORDS[2], 2), (PULSE_LDS_WORDS[2], 1)]:
        out.append(Case("pulse", "pulse_kernel", "", tables[key], ""))
    for nbins in (2, 65, 129):                                # the least bin count of every waves_per_block
        for form in ("hits", "no hits"):
            out.append(Case("fold", "fold_kernel", form, (nbins,), ""))
            out.append(Case("cand", "cand_fold_kernel", form, (nbins,), ""))
    for nbins in (2, 65, 129, 193):                           # ... and of every per_lane
        for form in ("stage 1, copy", "stage 1, no copy", "stage 2"):
            out.append(Case("cand", "cand_stage_kernel", form, (nbins,) + SEARCH_SMALL, ""))
    plans = {n: _smallest_ffa_plan(n) for n in (1, 2, 3)}
    for n in (1, 2, 3):
        out.append(Case("ffa", "ffa_pass", "the last of %d" % n, plans[n] + (1,), ""))
    out.append(Case("ffa", "ffa_pass", "not the last pass", plans[2] + (2,), ""))
    out.append(Case("ffa", "ffa_merge", "", plans[2] + (1 << plans[2][1],), ""))
    for log2n in LOG2NS:
        for form in ("voltages", "time", "channel"):
            out.append(Case("cdd", "cdd_kernel", form, (log2n,), ""))
    out.append(Case("clean", "clean_stats_kernel", "", (4,), ""))
    out.append(Case("clean", "clean_flags_kernel", "", (4,), ""))
    for w in ROW_WAVES:                                       # the least channel count of every row_waves
        nchan = min(m for m in range(4, 4097, 4) if row_waves(m) == w)
        for form in ("zero-DM", "no zero-DM"):
            out.append(Case("clean", "clean_apply_kernel", form, (nchan,), ""))
    out.append(Case("sift", "sift_score_kernel", "", "one event", ""))
    out.append(Case("sift", "sift_box_kernel", "", "random 5x3x7, the widest box", ""))
    out.append(Case("sift", "sift_list_kernel", "", "random 65x2x65, a list cut short", ""))
    return out


def _clean_class_nchans():
    """per row_threads 1 .. 1024 the channel count that fills it and the least one that pads it, where there is one"""
    out = []
    for k in range(11):
        G = 1 << k
        out.append(4 * G)
        if G >= 4:
            out.append(4 * (G // 2 + 1))
    return sorted(out)


PER_LANE_BORDERS = (64, 65, 128, 129, 192, 193)


def cand_classes(nbins):
    """the class a bin count falls into, where it stands at a border of per_lane"""
    return [("per_lane", per_lane(nbins), nbins)] if nbins in PER_LANE_BORDERS else []


def _class_cases():
    out = []
    for nchan in _clean_class_nchans():
        why = "; ".join(" ".join(str(v) for v in cl) for cl in clean_classes(nchan))
        out.append(Case("clean", "clean_apply_kernel", "zero-DM", (nchan,), why))
    for nbins in PER_LANE_BORDERS:
        out.append(Case("cand", "cand_stage_kernel", "stage 2", (nbins,) + SEARCH_BORDERS, "per_lane %d at %d bins" % (per_lane(nbins), nbins)))
    return out


INSTANTIATION_CASES = _instantiation_cases()
CLASS_CASES = _class_cases()
CASES = INSTANTIATION_CASES + CLASS_CASES


def by_library(lib):
    return [c for c in CASES if c.lib == lib]


def classes(c):
    """the geometry classes a run of case c takes"""
    return clean_classes(c.plan[0]) if c.lib == "clean" else cand_classes(c.plan[0]) if c.kernel == "cand_stage_kernel" else []


# every class there is: of the channel counts 4 .. 4096 and of the border bin counts
ALL_CLASSES = sorted({cl for m in range(4, 4097, 4) for cl in clean_classes(m)} | {cl for n in PER_LANE_BORDERS for cl in cand_classes(n)}, key=str)


def spell(t):
    """("cand_stage_kernel", (3, True)) -> "cand_stage_kernel<3, true>"; ("ffa_merge", ()) -> "ffa_merge" """
    if not t[1]:
        return t[0]
    return "%s<%s>" % (t[0], ", ".join(("true" if a else "false") if isinstance(a, bool) else str(a) for a in t[1]))


# What no comparison of an earlier suite reached, read once from those suites' own lists (the feature's channel counts of
# tests/test_clean_gpu.py, the refinement's bin counts of tests/test_cand_gpu.py, the width tables of tests/test_pulse_gpu.py,
# the shapes their other tests fix, and the lists of the other six suites, which between them had launched every
# instantiation of theirs): two instantiations -- the cleaning's rows of eight wavefronts, and the pulse search's tile of
# 1024 outputs in 64 KiB, which the pulse suite's assertion (every tile, every LDS size) let through because it never asked
# for the pairs --, the cleaning's classes below and three of the refinement's six border values.  (tests/test_clean_gpu.py's
# refusal test ends with one run of 8 channels that succeeds; nothing it writes is read.)  Committed as data: it is the
# record of what the matrix closed, and tests/test_search_family_matrix_cpu.py holds it to the model.
FIRST_LAUNCHED_HERE = (
    ("clean_apply_kernel", (8,)), ("pulse_kernel", (16384, 4)),
    ("row_threads", 2, "exact"), ("row_threads", 4, "exact"), ("row_threads", 8, "exact"), ("row_threads", 8, "padded"),
    ("row_threads", 16, "padded"), ("row_threads", 32, "exact"), ("row_threads", 32, "padded"), ("row_threads", 128, "exact"),
    ("row_threads", 256, "padded"), ("row_threads", 512, "exact"), ("row_threads", 512, "padded"), ("row_threads", 1024, "padded"),
    ("sort_len", 8), ("sort_len", 32), ("sort_len", 128), ("sort_len", 2048),
    ("flag_threads x keys", 64, 2), ("flag_threads x keys", 1024, 2),
    ("flag_lds > 65536", False, 2048), ("flag_lds > 65536", True, 2052),
    ("per_lane", 2, 128), ("per_lane", 3, 192), ("per_lane", 4, 193),
)

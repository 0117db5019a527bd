"""CPU suite of include/rtlws_fmfir.h (librtlws_fmfir.so): the ABI, the kernels' resources from the code-object
metadata, the refusals and their order, the LDS capacity statement of rtl-ws_amd/csrc/fmfir.h, the source rules, and --
on the restatement alone -- what the channel filter buys the discriminator.  No GPU is used."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ddcfir_ref
import fm_ref
import fmfir_ref
from test_abi_cpu import _declared_functions, _exported

P = ddcfir_ref.P
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rtl-ws_amd", "csrc")
NEW_SOURCES = ("fmfir.h", "fmfir_bank.hip", "fmfir_shim.hip", "ddcfir_ops.h", "fm_bank_stages.h")


def test_fmfir_library_exports_its_header_and_nothing_else(built):
    built.fmfir_lib()
    declared = _declared_functions("rtlws_fmfir.h")
    assert len(declared) == 7
    assert _exported(built.FMFIR_LIB) == set(declared)
    assert set(built.FMFIR_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.FMFIR_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    for other in ("librtlws_ddc.so", "librtlws_ddcfir.so", "librtlws_fm.so", "librtlws_fmbank.so"):
        assert other not in dyn, other                                        # a library of its own
    assert built.FMFIR_MAX_CHANNELS == built.FMBANK_MAX_CHANNELS == 32
    header = open(os.path.join(ROOT, "include", "rtlws_fmfir.h")).read()
    assert '#include "rtlws_ddcfir.h"' in header and "#define RTLWS_FMFIR_MAX_CHANNELS 32" in header


def test_fmfir_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the names are exactly the two instantiations of
    the launch table and the state copy; both bank kernels keep fm_bank.h's static LDS, and rtlws_fmfir_grid reports
    the threads and the LDS the code objects ask for."""
    from rtlws import codeobj
    built.fmfir_lib()
    ks = codeobj.kernels(built.FMFIR_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::(fmfir::fmfir_bank_kernel<(?:true|false)>|fmbank::fm_bank_state_copy_kernel)", d)
        assert m, d
        names[m.group(1)] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
    assert set(names) == {"fmfir::fmfir_bank_kernel<true>", "fmfir::fmfir_bank_kernel<false>", "fmbank::fm_bank_state_copy_kernel"}
    assert len(ks) == 3
    for name in ("fmfir::fmfir_bank_kernel<true>", "fmfir::fmfir_bank_kernel<false>"):
        assert names[name]["group_segment_fixed_size"] == 77056, name
    for r, l, name in ((8, 64, "true"), (4, 4, "true"), (128, 256, "true"), (10, 80, "false"), (7, 17, "false"), (8, 7, "false")):
        for nblocks, kernel in ((3, names["fmfir::fmfir_bank_kernel<%s>" % name]), (0, names["fmbank::fm_bank_state_copy_kernel"])):
            rc, blocks, threads, lds, tile = built.fmfir_grid(r, l, 9, 1030, nblocks)
            assert rc == 0 and tile > 0
            assert threads == kernel["max_flat_workgroup_size"], (r, l, nblocks, threads)
            assert lds == kernel["group_segment_fixed_size"], (r, l, nblocks, lds)
            assert 2 * lds <= 160 * 1024                                       # two workgroups per CU
            assert blocks == ((-(-3 * 257 // tile) + 1) * 2 if nblocks else 1)
    # the same geometry as the unfiltered bank's
    assert built.fmfir_grid(8, 8, 9, 1030, 3) == built.fmbank_grid(8, 9, 1030, 3)


def _constant(name, header):
    m = re.search(r"constexpr int %s = (\d+);" % name, open(os.path.join(CSRC, header)).read())
    return int(m.group(1))


def test_the_operands_fit_under_the_stage1_streams():
    """fmfir.h's capacity statement, swept: 1 KiB of operands per K step of 16 taps, at most 16 KiB, under the eight
    stage-1 streams; fmfir.h states it with a static_assert and adds nothing to fm_bank.h's LDS."""
    s1_bytes = _constant("COL_CH", "fm_bank.h") * 2 * _constant("S1_HALF", "fm_bank.h") * 4
    assert s1_bytes == 37888
    worst = 0
    for ntaps in range(1, 257):
        need = -(-ntaps // 16) * 64 * 16
        assert need <= s1_bytes, ntaps
        worst = max(worst, need)
    assert worst == 16 * 1024
    txt = open(os.path.join(CSRC, "fmfir.h")).read()
    assert "static_assert(operand_bytes(MAX_TAPS) == 16 * 1024 && operand_bytes(MAX_TAPS) <= COL_CH * fmbank::S1_CAP * 4" in txt
    assert "using fmbank::LDS_BYTES;" in txt and "__shared__" not in txt
    lds = _constant("COL_CH", "fm_bank.h") * (_constant("PHASE_CAP", "fm_bank.h") + 2 * _constant("S1_HALF", "fm_bank.h")) * 4
    assert lds == 77056


def test_new_sources_carry_no_conditionals_and_one_text_of_each_piece():
    """test_hooks_patch_applies' rule for the files of this library; the shared pieces defined once -- the operand
    builder and the window loader in ddcfir_ops.h, the tail range, a lane's phases and the half-band output in
    fm_bank_stages.h, compiled by both users --; and the rules this library's glue spells itself, in the words of
    the two existing shims, which stay the parent's files."""
    for f in NEW_SOURCES:
        txt = open(os.path.join(CSRC, f)).read()
        for m in re.finditer(r"^\s*#\s*(if|ifdef|ifndef|elif)\b(.*)$", txt, flags=re.M):
            assert m.group(2).strip().endswith("_H"), "%s: conditional on %r" % (f, m.group(2))
    every = {f: open(os.path.join(CSRC, f)).read() for f in os.listdir(CSRC)}
    for piece, home, users in (("uint4 filter_operand(", "ddcfir_ops.h", ("ddcfir_bank.hip", "fmfir_bank.hip")),
                               ("long load_window(", "ddcfir_ops.h", ("ddcfir_bank.hip", "fmfir_bank.hip")),
                               ("fm::TileRange tail_range(", "fm_bank_stages.h", ("fm_bank.hip", "fmfir_bank.hip")),
                               ("void emit_phase(", "fm_bank_stages.h", ("fm_bank.hip", "fmfir_bank.hip")),
                               ("float work_at(", "fm_bank_stages.h", ("fm_bank.hip", "fmfir_bank.hip")),
                               ("void fm_bank_state_copy_kernel(", "fm_bank_stages.h", ("fm_bank.hip", "fmfir_bank.hip"))):
        assert [f for f, txt in every.items() if piece in txt] == [home], piece
        for u in users:
            assert '#include "%s"' % home in every[u], (piece, u)
    # the kernel builds its tile maps as the host check of tests/fm_ref.py does
    txt = every["fmfir_bank.hip"].replace("fm::", "")
    for line in fm_ref.TILE_MAP_TEXT:
        assert txt.count(line) == 1, line
    # the family's rules come from ddc_plan.h; the two existing shims' own rules are spelled here in their words
    shim = every["fmfir_shim.hip"]
    assert '#include "ddc_plan.h"' in shim and "open_plan<rtlws_fmfir_plan>" in shim
    for rule in ("why_not_channels", "why_not_first", "fill_words", "why_not_capture", "why_not_plan"):
        assert "ddc::" + rule in shim, rule
    for other, texts in (("fmbank_shim.hip", ("block_len must be >= 20", "nblocks must be >= 0", "nblocks * block_len too large",
                                              "more tiles than one grid holds", "audio_stride must be >= nblocks * quarter",
                                              "null state pointer", "d_state_in and d_state_out must not overlap",
                                              "d_state_in, d_state_out and d_audio must be 4-byte aligned")),
                         ("ddcfir_shim.hip", ("decim must be 1 .. 128", "ntaps must be 1 .. 256", "out_shift must be 0 .. 30", "null taps",
                                              "a tap lies outside [-32639, 32639]"))):
        for text in texts:
            assert text in every[other] and text in shim, (other, text)


def test_fmfir_refusals_need_no_gpu(built):
    ok, need, grid = built.fmfir_supported, built.fmfir_samples_needed, built.fmfir_grid
    for r, l in ((1, 1), (7, 17), (8, 64), (12, 96), (128, 256), (3, 256), (16, 5)):
        for c in (1, 8, 9, 32):
            assert ok(r, l, c, 20, 0) == 1 and ok(r, l, c, 4102, 1000) == 1 and built.fmfir_last_error() == "", (r, l, c)
        assert need(r, l, 20, 0) == 0 and need(r, l, 23, 7) == (7 * 23 - 1) * r + l and built.fmfir_last_error() == ""
    bad = (((0, 8, 1, 20, 1), "decim"), ((129, 8, 1, 20, 1), "decim"), ((8, 0, 1, 20, 1), "ntaps"), ((8, 257, 1, 20, 1), "ntaps"),
           ((8, 8, 0, 20, 1), "nchannels"), ((8, 8, 33, 20, 1), "nchannels"), ((8, 8, 1, 19, 1), "block_len"),
           ((8, 8, 1, 20, -1), "nblocks"), ((8, 8, 32, 20, 1 << 40), "grid"), ((8, 8, 1, 20, 1 << 60), "too large"))
    for args, word in bad:
        assert ok(*args) == 0 and word in built.fmfir_last_error(), args
        assert grid(*args)[0] == -1 and word in built.fmfir_last_error(), args
        if word != "nchannels":
            assert need(args[0], args[1], args[3], args[4]) == -1 and word in built.fmfir_last_error(), args
    # the filter comes first, then the blocks, then the channels
    assert ok(0, 0, 0, 19, -1) == 0 and "decim" in built.fmfir_last_error()
    assert ok(8, 0, 0, 19, -1) == 0 and "ntaps" in built.fmfir_last_error()
    assert ok(8, 8, 0, 19, -1) == 0 and "block_len" in built.fmfir_last_error()
    assert ok(8, 8, 0, 20, -1) == 0 and "nblocks" in built.fmfir_last_error()

    t = grid(8, 8, 1, 20, 1)[4]
    bl = 4 * t
    for nb, c, want in ((1, 1, 2), (1, 8, 2), (1, 9, 4), (2, 32, 12), (3, 17, 12)):
        assert grid(8, 40, c, bl, nb)[:2] == (0, want), (nb, c)
    assert grid(8, 40, 1, bl + 4, 1)[:2] == (0, 3) and grid(8, 40, 5, bl, 0)[:4] == (0, 1, 256, 0)
    lib = built.fmfir_lib()
    assert lib.rtlws_fmfir_grid(8, 8, 1, 20, 1, None, None, None, None) == 0

    # open: the filter, the taps (rtlws_ddcfir_open's words), then the engine
    taps = np.full(8, 16384, np.int16)
    tp = taps.ctypes.data_as(ctypes.c_void_p)
    for args, word in (((None, 0, 8, tp), "decim"), ((None, 8, 257, tp), "ntaps"), ((None, 8, 8, None), "null taps"),
                       ((None, 8, 8, tp), "no CPU path")):
        assert not lib.rtlws_fmfir_open(*args) and word in built.fmfir_last_error(), word
    for value in (32640, -32640, -32768):
        wide = np.array([0, value, 0], np.int16)
        assert not lib.rtlws_fmfir_open(None, 8, 3, wide.ctypes.data_as(ctypes.c_void_p))
        why = built.fmfir_last_error()
        assert not built.ddcfir_lib().rtlws_ddcfir_open(None, 8, 3, wide.ctypes.data_as(ctypes.c_void_p))
        assert why.split(": ", 1)[1] == built.ddcfir_last_error().split(": ", 1)[1] and "[-32639, 32639]" in why
    edge = np.array([32639, -32639], np.int16)
    assert not lib.rtlws_fmfir_open(None, 8, 2, edge.ctypes.data_as(ctypes.c_void_p)) and "null engine" in built.fmfir_last_error()
    with pytest.raises(RuntimeError):
        built.FmFirPlan(None, 8, taps)
    lib.rtlws_fmfir_close(None)

    # every refusal of rtlws_fmfir_run is made before the plan is asked for anything, in this order
    A, SI, SO, AU = 1 << 20, 2 << 20, 3 << 20, 4 << 20        # stand-ins for device pointers: never dereferenced
    words = (ctypes.c_int * 32)(*([0] * 32))

    def run(**kw):
        args = [kw.get(k, d) for k, d in (("plan", None), ("iq", A), ("L", 40), ("nb", 3), ("first", 0), ("c", 2), ("w", words),
                                          ("shift", 14), ("si", SI), ("so", SO), ("audio", AU), ("stride", 30), ("st", None))]
        return lib.rtlws_fmfir_run(*args), built.fmfir_last_error()

    ordered = [({"L": 19}, "block_len"), ({"nb": -1}, "nblocks"), ({"c": 0}, "nchannels"),
               ({"L": 20, "nb": 1 << 40, "stride": 1 << 50, "c": 32}, "grid"), ({"first": -1}, "first_dec_index"),
               ({"shift": 31}, "out_shift"), ({"stride": 29}, "audio_stride"), ({"w": None}, "tuning_words"),
               ({"si": None}, "null state"), ({"so": SI}, "overlap"), ({"iq": None}, "null pointer"), ({"iq": A + 8}, "16-byte"),
               ({"si": SI + 2}, "4-byte"), ({}, "null plan")]
    for i, (kw, word) in enumerate(ordered):
        rc, why = run(**kw)
        assert rc == -1 and word in why and why.startswith("rtlws_fmfir_run: "), (kw, why)
        later = {}
        for kw2, _ in ordered[i + 1:]:                        # an earlier rule wins over every later one
            if set(kw2) & set(kw):
                continue
            later.update(kw2)
            rc, why = run(**dict(later, **kw))
            assert rc == -1 and word in why, (kw, later, why)
    for kw, word in (({"c": 33}, "nchannels"), ({"shift": -1}, "out_shift"), ({"audio": None}, "null pointer"),
                     ({"so": None}, "null state"), ({"so": SI + 2 * 84 - 4}, "overlap"), ({"si": SO + 84}, "overlap")):
        rc, why = run(**kw)
        assert rc == -1 and word in why, (kw, why)
    assert "null plan" in run(so=SI + 2 * 84)[1]                  # adjacent state ranges do not overlap
    assert "null plan" in run(nb=0, iq=None, audio=None)[1]       # a state copy needs neither capture nor audio
    assert "null plan" in run(shift=0)[1] and "null plan" in run(shift=30)[1]
    for bad_word in (P // 2, -P // 2 - 1, 1 << 20):
        rc, why = run(w=(ctypes.c_int * 2)(0, bad_word))
        assert rc == -1 and "tuning word" in why, bad_word
    assert "null plan" in run(w=(ctypes.c_int * 2)(-P // 2, P // 2 - 1))[1]
    assert "null plan" in run(w=(ctypes.c_int * 3)(0, 0, P))[1]   # a word behind nchannels is not read


def test_the_error_slot_is_its_own(built):
    """A refusal here leaves the other tuned-channel libraries' *_last_error() empty, and theirs leave this one's."""
    others = {"ddc": lambda: built.ddc_supported(8, 1), "fmbank": lambda: built.fmbank_supported(8, 1, 20, 1),
              "ddcfir": lambda: built.ddcfir_supported(8, 8, 1)}
    errs = {"ddc": built.ddc_last_error, "fmbank": built.fmbank_last_error, "ddcfir": built.ddcfir_last_error}
    for n, accept in others.items():
        assert accept() == 1 and errs[n]() == "", n
    assert built.fmfir_supported(8, 8, 0) == 0 and built.fmfir_last_error().startswith("rtlws_fmfir")
    for n in others:
        assert errs[n]() == "", n
    assert built.fmfir_supported(8, 8, 1) == 1 and built.fmfir_last_error() == ""
    assert built.ddc_supported(0, 1) == 0 and built.fmbank_supported(0, 1, 20, 1) == 0 and built.ddcfir_supported(0, 8, 1) == 0
    assert all(errs[n]() for n in others) and built.fmfir_last_error() == ""


def test_the_inputs_of_the_gpu_suite_are_what_it_says(built):
    """Conditions on tests/test_fmfir_gpu.py's data, checked without a device: the matrix covers the three load forms,
    both sides of a K step, L < R and both maxima; every multi-tile launch has the grid the suite asserts."""
    banks = [b[:3] for b in fmfir_ref.BANKS]
    forms = {"8-byte": lambda r, l: r % 4 == 0 and l % 4 == 0, "4-byte": lambda r, l: (r | l) % 2 == 0 and (r % 4 or l % 4),
             "2-byte": lambda r, l: (r | l) % 2 == 1}
    for name, form in forms.items():
        assert any(form(r, l) for r, l, _ in banks), name
    assert (12, 16, 8) in banks and (12, 17, 8) in banks and (128, 256, 32) in banks and any(l < r for r, l, _ in banks)
    tile = built.fmfir_grid(8, 8, 1, 20, 1)[4]
    for case, r, l, c in fmfir_ref.tile_bank_runs(tile):
        rc, blocks, _, _, t = built.fmfir_grid(r, l, c, case.block_len, case.nblocks)
        assert rc == 0 and t == tile and blocks == (case.ntiles(tile) + 1) * -(-c // 8), (case.id, r, l, c)


# ---- stage A at the window forms of the filtered down-converter (tests/fmfir_ref.py's stage_a_matrix) ----------------
# The restatement and the oracle's chain take about 5.4 ns per unit of ntaps * channels * nblocks * block_len (0.18 s at
# the largest product of the matrix, 33 390 592); three seconds are 5.5e8 units.  No case comes near it, so no channel
# count had to be moved to a shorter block shape.
PRODUCT_BOUND = 550_000_000


def _stage_a_conditions(matrix, tile):
    """What the stage-A matrix has to meet, per instantiation: raises AssertionError."""
    pairs = fmfir_ref.stage_a_pairs()
    assert sorted((c.R, c.L) for c in matrix) == sorted(pairs) and len(set(pairs)) == len(pairs)
    assert set(pairs) >= {(R, L) for R in ddcfir_ref.R_AXIS for L in ddcfir_ref.l_axis(R)}
    shapes = set(fmfir_ref.stage_a_shapes(tile))
    for inst in (True, False):
        mine = [c for c in matrix if c.aligned == inst]
        assert {c.C for c in mine} == set(fmfir_ref.STAGE_A_C) == {1, 2, 8, 9, 17, 24, 32}, inst
        assert {c.shift for c in mine} == {0, 9, 14} and {c.first for c in mine} == {0, 123456789, (1 << 40) + 12345}, inst
        assert {c.bytes for c in mine} == {"random", "full scale"} and {c.taps for c in mine} == {"random", "+max", "-max"}, inst
        assert {(c.block_len, c.nblocks) for c in mine} == shapes, inst
        assert {c.L % 16 for c in mine} == {L % 16 for R, L in pairs if ddcfir_ref.aligned(R, L) == inst}, inst
        assert {-(-c.L // 16) for c in mine} >= {1, 2, 16}, inst
        reached = {r for c in mine for r in fmfir_ref.np_residues(c, tile)}
        for name, residues in fmfir_ref.NP_CLASSES.items():
            assert reached & set(residues), (inst, name)
        # more than one column tile over more than one tile, and a first_dec_index whose upper bits the lookup drops
        assert any(c.C > 8 and c.nblocks * (c.block_len // 4) > tile for c in mine), inst
        assert any(c.first >> 16 and c.nblocks * (c.block_len // 4) > tile for c in mine), inst


def test_the_stage_a_matrix_meets_its_conditions(built):
    """Per instantiation: every value of every axis, every ntaps mod 16 of the pairs, 1, 2 and 16 K steps, and ordinary
    tiles whose np mod 32 lies in each of 1 .. 15, 16, 17 .. 31 and 0 (the last pair of row tiles: one partly live; one
    full and one dead; one full and one partly live; both full).  Deleting any one (decim, ntaps), and taking away
    the launches that reach any one class of np, fails.  The restatement's cost stays under its bound."""
    tile = built.fmfir_grid(8, 8, 1, 20, 1)[4]
    matrix = fmfir_ref.stage_a_matrix(tile)
    _stage_a_conditions(matrix, tile)
    assert len(matrix) == 61 and sum(c.aligned for c in matrix) == 12
    assert len({c.id for c in matrix}) == len(matrix)
    for i in range(len(matrix)):
        with pytest.raises(AssertionError):
            _stage_a_conditions(matrix[:i] + matrix[i + 1:], tile)
    for name, residues in fmfir_ref.NP_CLASSES.items():
        without = [c for c in matrix if not set(fmfir_ref.np_residues(c, tile)) & set(residues)]
        assert len(without) < len(matrix)
        with pytest.raises(AssertionError):
            _stage_a_conditions(without, tile)
    # what the axes of the ddcfir suite alone would leave out under the aligned instantiation
    assert {-(-L // 16) for R in ddcfir_ref.R_AXIS for L in ddcfir_ref.l_axis(R) if ddcfir_ref.aligned(R, L)} == {1, 4, 6, 8, 16}
    assert [(R, L, ddcfir_ref.aligned(R, L), -(-L // 16)) for R, L in fmfir_ref.STAGE_A_EXTRA] == [(8, 24, True, 2)]
    # L = 255, L = R + 1 and L = 1 at every R; a launch per shape of fm_ref.tile_cases that the issue names
    for R in ddcfir_ref.R_AXIS:
        assert {1, R + 1, 255} <= {c.L for c in matrix if c.R == R}, R
    largest = max(matrix, key=lambda c: c.product)
    print("largest ntaps * channels * nblocks * block_len: %d at %s; bound %d" % (largest.product, largest.id, PRODUCT_BOUND))
    assert largest.product <= PRODUCT_BOUND and largest.product == 33390592, largest.product
    for c in matrix:
        assert built.fmfir_supported(c.R, c.L, c.C, c.block_len, c.nblocks) == 1, c.id
    comp = fmfir_ref.composition_cases(tile)
    assert [matrix[i].aligned for i in comp] == [True, False]


# ---- why the filter matters, end to end: measured on tests/fmfir_ref.py's restatement --------------
# measured: boxcar -0.17 dB (the error is as strong as the wanted tone), designed 8R = 96-tap filter -44.69 dB; each is
# asserted with 6 dB of margin on its own side
BOXCAR_AT_LEAST_DB = -0.17 - 6.0
FILTERED_AT_MOST_DB = -44.69 + 6.0


def test_the_filter_keeps_the_neighbour_out_of_the_audio(oracle):
    """An FM-modulated tone on the channel's centre and a carrier three times as strong 1.5 output bandwidths away, at
    ddcfir_ref.SELECTIVITY_R: the audio's error against the interferer-free run, in dB of the wanted tone."""
    r = fmfir_ref.FM_R
    assert fmfir_ref.FM_WANTED_AMP + fmfir_ref.FM_INTERFERER_AMP <= 127
    boxcar = fmfir_ref.audio_error_db(oracle, ddcfir_ref.boxcar(r))
    filtered = fmfir_ref.audio_error_db(oracle, ddcfir_ref.design(r, 8 * r))
    print("audio error behind the boxcar %.2f dB, behind the designed %d-tap filter %.2f dB" % (boxcar, 8 * r, filtered))
    assert boxcar >= BOXCAR_AT_LEAST_DB                    # visibly disturbed
    assert filtered <= FILTERED_AT_MOST_DB
    assert filtered <= boxcar - 20.0

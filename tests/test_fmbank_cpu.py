"""CPU suite of include/rtlws_fmbank.h (librtlws_fmbank.so): the ABI, the kernels' resources from the code-object
metadata, the refusals, the one table builder, the LDS capacities of rtl-ws_amd/csrc/fm_bank.h against the stream
maps, and the conditions on the inputs of tests/test_fmbank_gpu.py.  No GPU is used."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import ddc_ref
import fm_ref
import fmbank_ref
from test_abi_cpu import _declared_by_lib, _declared_functions, _exported

P = ddc_ref.P
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rtl-ws_amd", "csrc")


def test_fmbank_library_exports_its_header_and_nothing_else(built):
    built.fmbank_lib()
    declared = _declared_functions("rtlws_fmbank.h")
    assert len(declared) == 6
    assert _exported(built.FMBANK_LIB) == set(declared)
    assert set(built.FMBANK_SYMBOLS) == set(declared)
    dyn = subprocess.run(["readelf", "-d", built.FMBANK_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn
    assert "librtlws_ddc.so" not in dyn and "librtlws_fm.so" not in dyn          # a library of its own
    # the existing libraries export what they exported
    for lib, names in _declared_by_lib().items():
        assert _exported(getattr(built, lib)) == set(names), lib
    for lib, header in (("FM_LIB", "rtlws_fm.h"), ("DDC_LIB", "rtlws_ddc.h"), ("LONG_LIB", "rtlws_long.h"),
                        ("ANYLEN_LIB", "rtlws_anylen.h")):
        assert _exported(getattr(built, lib)) == set(_declared_functions(header)), lib
    assert built.FMBANK_MAX_CHANNELS == built.DDC_MAX_CHANNELS == 32


def test_fmbank_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the kernel names are exactly the instantiations
    the launch table reaches (R = 8, 10, 12, the generic one, the state copy); rtlws_fmbank_grid reports the
    threads and the LDS the code objects ask for."""
    from rtlws import codeobj
    built.fmbank_lib()
    ks = codeobj.kernels(built.FMBANK_LIB)
    names = {}
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::fmbank::(fm_bank_kernel<\d+>|fm_bank_state_copy_kernel)", d)
        assert m, d
        names[m.group(1)] = k
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
    assert set(names) == {"fm_bank_kernel<%d>" % r for r in (0, 8, 10, 12)} | {"fm_bank_state_copy_kernel"} and len(ks) == 5
    for r, name in ((8, "fm_bank_kernel<8>"), (10, "fm_bank_kernel<10>"), (12, "fm_bank_kernel<12>"),
                    (7, "fm_bank_kernel<0>"), (128, "fm_bank_kernel<0>")):
        for nblocks, kernel in ((3, names[name]), (0, names["fm_bank_state_copy_kernel"])):
            rc, blocks, threads, lds, tile = built.fmbank_grid(r, 9, 1030, nblocks)
            assert rc == 0 and tile > 0
            assert threads == kernel["max_flat_workgroup_size"], (r, nblocks, threads)
            assert lds == kernel["group_segment_fixed_size"], (r, nblocks, lds)
            assert lds <= 160 * 1024
            assert blocks == ((-(-3 * 257 // tile) + 1) * 2 if nblocks else 1)


def test_fmbank_refusals_need_no_gpu(built):
    ok = built.fmbank_supported
    for r in (1, 7, 8, 10, 12, 16, 17, 128):
        for c in (1, 8, 9, 32):
            assert ok(r, c, 20, 0) == 1 and ok(r, c, 4102, 1000) == 1 and built.fmbank_last_error() == "", (r, c)
    for args, word in (((0, 1, 20, 1), "cic_r"), ((129, 1, 20, 1), "cic_r"), ((8, 0, 20, 1), "nchannels"),
                       ((8, 33, 20, 1), "nchannels"), ((8, 1, 19, 1), "block_len"), ((8, 1, 20, -1), "nblocks"),
                       ((8, 32, 20, 1 << 40), "grid")):
        assert ok(*args) == 0 and word in built.fmbank_last_error(), args

    # the grid at a tile border: per column tile the audio tiles and the one workgroup of the states
    t = built.fmbank_grid(8, 1, 20, 1)[4]
    assert t > 0 and t % 2 == 0
    L = 4 * t                                                 # quarter = t
    for nb, c, want in ((1, 1, 2), (1, 8, 2), (1, 9, 4), (2, 32, 12), (3, 17, 12)):
        assert built.fmbank_grid(8, c, L, nb)[:2] == (0, want), (nb, c)
    assert built.fmbank_grid(8, 1, L + 4, 1)[:2] == (0, 3)
    assert built.fmbank_grid(8, 1, 19, 1)[0] == -1 and built.fmbank_grid(8, 33, 20, 1)[0] == -1
    lib = built.fmbank_lib()
    assert lib.rtlws_fmbank_grid(8, 1, 20, 1, None, None, None, None) == 0

    # no engine, no plan: a text, never a crash
    assert not lib.rtlws_fmbank_open(None) and "no CPU path" in built.fmbank_last_error()
    with pytest.raises(RuntimeError):
        built.FmBankPlan(None)
    lib.rtlws_fmbank_close(None)

    # every refusal of rtlws_fmbank_run is made before the plan is asked for anything
    A, SI, SO, AU = 1 << 20, 2 << 20, 3 << 20, 4 << 20        # stand-ins for device pointers: never dereferenced
    words = (ctypes.c_int * 32)(*([0] * 32))

    def run(**kw):
        args = [kw.get(k, d) for k, d in (("plan", None), ("r", 8), ("iq", A), ("L", 40), ("nb", 3), ("first", 0), ("c", 2),
                                          ("w", words), ("si", SI), ("so", SO), ("audio", AU), ("stride", 30), ("st", None))]
        return lib.rtlws_fmbank_run(*args), built.fmbank_last_error()

    for kw, word in (({"r": 0}, "cic_r"), ({"r": 129}, "cic_r"), ({"c": 0}, "nchannels"), ({"c": 33}, "nchannels"),
                     ({"L": 19}, "block_len"), ({"nb": -1}, "nblocks"), ({"first": -1}, "first_dec_index"),
                     ({"stride": 29}, "audio_stride"), ({"w": None}, "tuning_words"), ({"iq": None}, "null pointer"),
                     ({"audio": None}, "null pointer"), ({"si": None}, "null state"), ({"so": None}, "null state"),
                     ({"so": SI}, "overlap"), ({"so": SI + 2 * 84 - 4}, "overlap"), ({"si": SO + 84}, "overlap"),
                     ({"iq": A + 8}, "16-byte"), ({"L": 20, "nb": 1 << 40, "stride": 1 << 50, "c": 32}, "grid"),
                     ({}, "null plan")):
        rc, why = run(**kw)
        assert rc == -1 and word in why, (kw, why)
    assert "null plan" in run(so=SI + 2 * 84)[1]                  # adjacent state ranges do not overlap
    assert "null plan" in run(nb=0, iq=None, audio=None)[1]       # a state copy needs neither capture nor audio
    for bad in (P // 2, -P // 2 - 1, 1 << 20):
        w = (ctypes.c_int * 2)(0, bad)
        rc, why = run(w=w)
        assert rc == -1 and "tuning word" in why, bad
    w = (ctypes.c_int * 2)(-P // 2, P // 2 - 1)                   # the ends of the range pass that check
    assert "null plan" in run(w=w)[1]
    w = (ctypes.c_int * 3)(0, 0, P)                               # a word behind nchannels is not read
    assert "null plan" in run(w=w)[1]


def test_one_table_builder_and_it_equals_numpy(built, tmp_path):
    """rtl-ws_amd/csrc/ddc_table.h is the only builder of the phasor table: both libraries' glue calls it -- through
    the one open of csrc/ddc_plan.h --, it is compiled here on its own and gives tests/ddc_ref.py's table, as
    rtlws_ddc_table does."""
    plan = open(os.path.join(CSRC, "ddc_plan.h")).read()
    assert '#include "ddc_table.h"' in plan and "build_table(host.data(), P)" in plan
    assert "lrint" not in plan and "std::cos" not in plan
    for shim in ("ddc_shim.hip", "fmbank_shim.hip"):
        txt = open(os.path.join(CSRC, shim)).read()
        assert '#include "ddc_plan.h"' in txt and "open_plan<rtlws_" in txt, shim
        assert "lrint" not in txt and "std::cos" not in txt, shim
    src = tmp_path / "table.cpp"
    src.write_text('#include "ddc_table.h"\nextern "C" void table(short* t, int p) { rtlws::ddc::build_table(t, p); }\n')
    so = tmp_path / "table.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-I", CSRC, str(src), "-o", str(so)], check=True)
    got = np.empty((P, 2), dtype=np.int16)
    ctypes.CDLL(str(so)).table(got.ctypes.data_as(ctypes.c_void_p), P)
    assert np.array_equal(got, ddc_ref.table())
    assert np.array_equal(built.ddc_table(), ddc_ref.table())


def _constants():
    txt = open(os.path.join(CSRC, "fm_bank.h")).read()
    val = {}
    for name in ("TILE", "THREADS", "PHASE_CAP", "S1_HALF", "S2_HALF", "COL_CH"):
        val[name] = int(re.search(r"constexpr int %s = (\d+);" % name, txt).group(1))
    return val


def _worst_tile_ranges(tile):
    """the largest (n2, n1, np) over every block_len 20 .. 4200 and every tile of enough blocks for three tiles"""
    worst = [0, 0, 0]
    for L in range(20, 4201):
        quarter = L // 4
        nb = -(-3 * tile // quarter) + 1
        for t in range(-(-nb * quarter // tile)):
            r = fm_ref.tile_range(t, L, nb, tile)
            worst = [max(a, b) for a, b in zip(worst, r)]
    return worst


def test_capacities_hold_for_every_block_shape(built):
    """With the library's own tile, what a tile reads of each stream (tests/fm_ref.py's tile_range) stays within
    fm_bank.h's capacities for every block_len 20 .. 4200, over enough blocks for three tiles."""
    k = _constants()
    rc, _, threads, lds, tile = built.fmbank_grid(8, 8, 20, 1)
    assert rc == 0 and tile == k["TILE"] and threads == k["THREADS"]
    assert lds == k["COL_CH"] * (k["PHASE_CAP"] + 2 * k["S1_HALF"]) * 4
    n2, n1, nph = _worst_tile_ranges(tile)
    print("tile %d: n2 <= %d, n1 <= %d, phases <= %d" % (tile, n2, n1, nph))
    assert n2 == 2 * tile + 9
    assert (n2 + 1) // 2 <= k["S2_HALF"] and k["S2_HALF"] + n2 // 2 <= k["PHASE_CAP"]
    assert (n1 + 1) // 2 <= k["S1_HALF"]
    assert nph <= k["PHASE_CAP"]


# ---- the block shapes tests/test_fmbank_gpu.py launches over several tiles (fm_ref.tile_cases) -------------------

def _tile(built):
    rc, _, _, _, tile = built.fmbank_grid(8, 1, 20, 1)
    assert rc == 0
    return tile


def test_multi_tile_cases_meet_their_conditions(built):
    """tests/test_fm_cpu.py's test of the same name with this library's tile: four tiles or more and a partial last
    one, a map origin in a later block with a border behind it wherever a map skips, regime b's borders in the halos,
    and the block_len = 23 case at the largest ranges any block shape reaches."""
    k = _constants()
    tile = _tile(built)
    worst = _worst_tile_ranges(tile)
    for line in fm_ref.case_report(tile, worst):
        print(line)
    print("tile %d, block_len 23 fills %d of %d phase slots, %d of %d per stage-1 half"
          % (tile, worst[2], k["PHASE_CAP"], (worst[1] + 1) // 2, k["S1_HALF"]))
    for c, R, C in fmbank_ref.tile_bank_runs(tile):
        rc, blocks, _, _, t = built.fmbank_grid(R, C, c.block_len, c.nblocks)
        assert rc == 0 and t == tile and blocks == (c.ntiles(tile) + 1) * -(-C // 8), (c.id, R, C)


def test_multi_tile_inputs_reach_both_sides_of_the_limiter(oracle, built):
    """On the reference alone: in every launch of the multi-tile suite every channel's demodulator output holds clamped
    and unclamped samples."""
    for c, R, C in fmbank_ref.tile_bank_runs(_tile(built)):
        iq, words, states = fmbank_ref.case_inputs(c, R, C)
        streams = ddc_ref.ddc_ref(iq, R, words)
        for ch in range(C):
            d = oracle.fm_demod(streams[ch], prev_phase=float(states[ch][0]))[0]
            assert np.any(np.abs(d) == 1.0) and np.any(np.abs(d) < 1.0), (c.id, R, C, ch)


@pytest.fixture(scope="module")
def host_maps(built, tmp_path_factory):
    cc = fm_ref.host_compiler()
    if cc is None:
        pytest.skip("no C++ compiler for the host")
    return fm_ref.HostMaps(cc, CSRC, tmp_path_factory.mktemp("maps"), _tile(built))


def test_tile_map_equals_maps_in_the_product_text(host_maps):
    """fm_maps.h compiled for the host with this library's tile: TileMap, Maps and fm_ref's numpy maps agree at every
    position every tile reads, for every block_len 20 .. 4200."""
    print("tile %d: %d positions" % (host_maps.tile, fm_ref.sweep_host_maps(host_maps)))


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_tile_map_beyond_32_bits(host_maps, residue):
    fm_ref.check_host_maps_beyond_32_bits(host_maps, residue)


def test_wrong_tile_maps_pass_the_earlier_shapes_and_fail_the_new_ones(built):
    fm_ref.check_wrong_tile_maps(_tile(built))


def test_inputs_of_the_gpu_suite_reach_every_branch(oracle):
    """A condition on the test data, checked on the reference alone: in ddc_ref's streams of the branch captures
    both sides of the limiter and every branch of atan2_approx occur."""
    caps = fmbank_ref.branch_captures()
    streams = ddc_ref.ddc_ref(caps["axes"], fmbank_ref.BRANCH_R, fmbank_ref.branch_words())
    assert not ddc_ref.ddc_ref(caps["all128"], fmbank_ref.BRANCH_R, fmbank_ref.branch_words()).any()
    x = streams[..., 0].astype(np.float32).ravel()
    y = streams[..., 1].astype(np.float32).ravel()
    nz = x != 0
    z = np.abs(y[nz] / x[nz])
    seen = {"|z| < 1": np.any(z < 1), "|z| >= 1": np.any(z >= 1),
            "x < 0, y < 0": np.any((x < 0) & (y < 0)), "x < 0, y >= 0": np.any((x < 0) & (y >= 0)),
            "|z| < 1, x < 0, y < 0": np.any((x[nz] < 0) & (y[nz] < 0) & (z < 1)),
            "|z| < 1, x < 0, y >= 0": np.any((x[nz] < 0) & (y[nz] >= 0) & (z < 1)),
            "|z| >= 1, y < 0": np.any((y[nz] < 0) & (z >= 1)),
            "x == 0, y > 0": np.any(~nz & (y > 0)), "x == 0, y == 0": np.any(~nz & (y == 0)),
            "x == 0, y < 0": np.any(~nz & (y < 0))}
    assert all(seen.values()), seen
    # the x == 0 samples are the word-0 channel's, as built
    x0 = streams[0, :, 0] == 0
    assert np.any(x0 & (streams[0, :, 1] > 0)) and np.any(x0 & (streams[0, :, 1] < 0)) and np.any(x0 & (streams[0, :, 1] == 0))
    for c in range(streams.shape[0]):
        d = oracle.fm_demod(streams[c])[0]
        assert np.any(np.abs(d) == 1.0) and np.any(np.abs(d) < 1.0), c

"""CPU suite of include/rtlws_fm.h (librtlws_fm.so): the ABI, the kernels' resources from the code-object metadata,
the refusals, and the fused kernel's two stream maps restated in numpy against the oracle.  No GPU is used."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fm_ref
from test_abi_cpu import _declared_functions, _exported, ROOT


def test_fm_library_exports_its_header_and_nothing_else(built):
    built.fm_lib()
    declared = _declared_functions("rtlws_fm.h")
    assert len(declared) == 6
    assert _exported(built.FM_LIB) == set(declared)
    assert set(built.FM_SYMBOLS) == set(declared)
    # the drop-in library (audio_main.h) depends on it and finds it beside itself
    dyn = subprocess.run(["readelf", "-d", built.AMD_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_fm.so" in dyn and "$ORIGIN" in dyn
    dyn = subprocess.run(["readelf", "-d", built.FM_LIB], capture_output=True, text=True, check=True).stdout
    assert "librtlws_hip.so" in dyn and "$ORIGIN" in dyn


def test_fm_kernels_do_not_spill(built):
    """Every kernel of the library: no scratch, no spilled register; the tile kernels fit at least six
    workgroups of four wavefronts on a compute unit (<= 80 VGPRs, 160 KiB of LDS)."""
    from rtlws import codeobj
    built.fm_lib()
    ks = codeobj.kernels(built.FM_LIB)
    names = set()
    for k in ks:
        d = k.get("demangled", k["name"])
        m = re.search(r"rtlws::fm::(fm_chain_kernel<\d+, (?:true|false)>|fm_state_copy_kernel)", d)
        assert m, d
        names.add(m.group(1))
        assert k["vgpr_spill_count"] == 0 and k["private_segment_fixed_size"] == 0, d
        assert not k.get("sgpr_spill_count", 0), d
        if "true>" in m.group(1):
            assert k["vgpr_count"] + k.get("agpr_count", 0) <= 80, d
            assert 6 * k["group_segment_fixed_size"] <= 160 * 1024, d
            assert k["max_flat_workgroup_size"] == 256
    want = {"fm_chain_kernel<%d, %s>" % (s, r) for s in (0, 1, 8, 10, 12) for r in ("true", "false")}
    assert names == want | {"fm_state_copy_kernel"}
    rc, blocks, threads, lds, tile = built.fm_grid(1024, 64, 8)
    assert rc == 0 and threads == 256 and tile == 512 and blocks == 64 * 256 // tile + 1
    assert {k["group_segment_fixed_size"] for k in ks if "true>" in k.get("demangled", "")} == {lds}


def test_fm_sources_follow_the_csrc_rules():
    """One text of atan2_approx and of the half-band expression (csrc/fm_math.h, included by both users); the new
    files are built without contraction."""
    csrc = os.path.join(ROOT, "rtl-ws_amd", "csrc")
    for f in ("resample_kernels.hip", "fm_chain.hip"):
        txt = open(os.path.join(csrc, f)).read()
        assert '#include "fm_math.h"' in txt, f
        assert "0.28f" not in txt and "0.34790f" not in txt, f
    math = open(os.path.join(csrc, "fm_math.h")).read()
    assert math.count("0.28f") == 2 and math.count("0.34790f") == 1
    mk = open(os.path.join(ROOT, "rtl-ws_amd", "Makefile")).read()
    assert re.search(r"fm_chain\.o:.*\n\t\$\(HIPCC\) \$\(HIPFLAGS\) -ffp-contract=off", mk)


def test_fm_refusals_need_no_gpu(built):
    ok = built.fm_supported
    for L in (20, 21, 23, 1024, 19200, 1 << 24):
        for r in (0, 1, 7, 8, 10, 12, 128):
            assert ok(L, 1, r) == 1 and built.fm_last_error() == "", (L, r)
    assert ok(20, 0, 0) == 1
    why = {}
    for name, args in (("short", (19, 1, 0)), ("neg", (20, -1, 0)), ("r129", (20, 1, 129)), ("rneg", (20, 1, -1)),
                       ("huge", (1 << 30, 1 << 40, 0))):
        assert ok(*args) == 0, name
        why[name] = built.fm_last_error()
    assert "block_len" in why["short"] and "nblocks" in why["neg"] and "cic_r" in why["r129"] and "cic_r" in why["rneg"]
    assert why["huge"]
    assert built.fm_grid(19, 1, 0)[0] == -1 and built.fm_grid(20, 1, 200)[0] == -1
    assert built.fm_grid(20, 0, 0)[:2] == (0, 1)

    # the launching entry points: every refusal of the header is made before a device is asked for anything
    L = built.fm_lib()
    A, B, S1, S2 = 1 << 20, 2 << 20, 3 << 20, (3 << 20) + 128       # stand-ins for device pointers: never dereferenced
    eng = 1 << 12                                                   # nor is the engine, on a refused call
    cs32 = lambda **kw: L.rtlws_fm_audio_blocks(*[kw.get(k, d) for k, d in (
        ("e", eng), ("iq", A), ("L", 1024), ("nb", 2), ("si", S1), ("so", S2), ("run2", 1), ("audio", B), ("st", None))])
    cu8 = lambda **kw: L.rtlws_fm_audio_blocks_cu8(*[kw.get(k, d) for k, d in (
        ("e", eng), ("r", 8), ("iq", A), ("L", 1024), ("nb", 2), ("si", S1), ("so", S2), ("run2", 1), ("audio", B),
        ("dec", None), ("st", None))])
    for fn in (cs32, cu8):
        assert fn(L=19) == -1 and "block_len" in built.fm_last_error()
        assert fn(nb=-1) == -1
        assert fn(iq=None) == -1 and fn(si=None) == -1 and fn(so=None) == -1 and fn(audio=None) == -1
        assert fn(so=S1) == -1 and "differ" in built.fm_last_error()
        assert fn(e=None) == -1 and "no CPU path" in built.fm_last_error()
    assert cs32(iq=A + 4) == -1 and "8-byte" in built.fm_last_error()
    assert cu8(iq=A + 8) == -1 and "16-byte" in built.fm_last_error()
    assert cu8(dec=B + 4) == -1 and "8-byte" in built.fm_last_error()
    assert cu8(r=0) == -1 and cu8(r=129) == -1
    assert L.rtlws_fm_prepare(None) == -1


def test_fm_without_a_gpu_fails_loudly(built):
    """There is no CPU path: no engine, no audio."""
    if built.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError):
        built.Engine(0)
    L = built.fm_lib()
    iq = np.zeros((1024, 2), dtype=np.int32)
    st = np.zeros(2 * 24, dtype=np.float32)
    audio = np.full(256, 7.0, dtype=np.float32)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    rc = L.rtlws_fm_audio_blocks(None, p(iq), 1024, 1, p(st), p(st[24:]), 1, p(audio), None)
    assert rc == -1 and "no CPU path" in built.fm_last_error()
    assert np.all(audio == 7.0) and not st.any()                    # nothing was computed on the host


@pytest.mark.parametrize("block_len", [20, 22, 23, 25, 1024])
def test_stream_maps_equal_the_per_block_chain(oracle, block_len):
    """fm_chain.hip's claim: nblocks calls of audio_fm_demodulator are one continuous filter over concatenated,
    truncated streams.  3 blocks, random state in; audio and all 21 floats of the state, bit for bit."""
    nb = 3
    for kind, make in (("A", fm_ref.input_a), ("B", fm_ref.input_b)):
        iq = make(block_len * nb, seed=block_len)
        st = fm_ref.random_state(block_len + 1)
        want, want_st = fm_ref.oracle_chain(oracle, iq, block_len, st)
        got, got_st = fm_ref.chain_by_maps(oracle, iq, block_len, st)
        assert want.size == nb * (block_len // 4)
        assert np.array_equal(got, want), kind
        assert np.array_equal(got_st, want_st), (kind, np.nonzero(got_st != want_st))


def _worst_tile_ranges(tile):
    """the largest (n2, n1, np) over every block shape and every tile index"""
    worst = [0, 0, 0]
    for L in list(range(20, 120)) + [1023, 1026, 4102, 19200]:
        quarter = L // 4
        nb = (6 * tile) // quarter + 2
        ntiles = (nb * quarter + tile - 1) // tile
        for t in range(ntiles):
            r = fm_ref.tile_range(t, L, nb, tile)
            worst = [max(a, b) for a, b in zip(worst, r)]
    return worst


def _capacities():
    hdr = open(os.path.join(ROOT, "rtl-ws_amd", "csrc", "fm_chain.h")).read()
    const = lambda n: int(re.search(r"constexpr int %s = (\d+);" % n, hdr).group(1))
    return const("TILE"), const("PHASE_CAP"), const("S1_HALF"), const("S2_HALF")


def test_tile_ranges_fit_the_lds_capacities(built):
    """What a tile reads of each stream (tile_range() of fm_chain.hip, restated in fm_ref.tile_range) stays inside
    the capacities of fm_chain.h for every block shape -- the worst is block_len = 23 -- and every tile index."""
    tile, phase_cap, s1_half, s2_half = _capacities()
    assert built.fm_grid(20, 1, 0)[4] == tile
    assert s1_half % 32 == 16 and s2_half % 32 == 16               # even / odd halves 16 banks apart
    n2, n1, np_ = _worst_tile_ranges(tile)
    print("worst n2 %d, n1 %d, phases %d" % (n2, n1, np_))
    assert (n2 + 1) // 2 <= s2_half and 2 * s2_half <= phase_cap
    assert (n1 + 1) // 2 <= s1_half and np_ <= phase_cap


# ---- the block shapes tests/test_fm_gpu.py launches over several tiles (fm_ref.tile_cases) -----------------------

def test_multi_tile_cases_meet_their_conditions(built):
    """From the model alone, with the library's own tile: every case has four tiles or more and a partial last one;
    where a map skips, some tile behind the first has its map's origin in a later block and a block border inside
    what it reads; regime b's borders lie in the halos of tiles 1, 2 (stage 2) and 3 (stage 1); the block_len = 23
    case reaches the largest ranges any block shape reaches, so its launch fills LDS as far as any can."""
    tile = built.fm_grid(20, 1, 0)[4]
    _, phase_cap, s1_half, _ = _capacities()
    for line in fm_ref.case_report(tile, _worst_tile_ranges(tile)):
        print(line)
    n2, n1, nph = _worst_tile_ranges(tile)
    print("tile %d, block_len 23 fills %d of %d phase slots, %d of %d per stage-1 half" % (tile, nph, phase_cap, (n1 + 1) // 2, s1_half))
    for c in fm_ref.tile_cases(tile):
        rc, blocks, _, _, t = built.fm_grid(c.block_len, c.nblocks, 0)
        assert rc == 0 and t == tile and blocks == c.ntiles(tile) + 1, c.id


@pytest.mark.parametrize("kind", ["A", "B"])
def test_multi_tile_inputs_reach_both_sides_of_the_limiter(oracle, built, kind):
    """On the oracle alone: in every case of tests/test_fm_gpu.py's multi-tile suite between 10 % and 90 % of the
    demodulator's outputs are clamped."""
    make = {"A": fm_ref.input_a, "B": fm_ref.input_b}[kind]
    for c in fm_ref.tile_cases(built.fm_grid(20, 1, 0)[4]):
        iq, st = fm_ref.case_input(make, c)
        clamped = np.mean(np.abs(oracle.fm_demod(iq, prev_phase=float(st[0]))[0]) == 1.0)
        print("input %s, case %s: %.1f %% of %d samples clamped" % (kind, c.id, 100 * clamped, iq.shape[0]))
        assert 0.10 <= clamped <= 0.90, c.id


@pytest.fixture(scope="module")
def host_maps(built, tmp_path_factory):
    cc = fm_ref.host_compiler()
    if cc is None:
        pytest.skip("no C++ compiler for the host")
    tile = built.fm_grid(20, 1, 0)[4]
    return fm_ref.HostMaps(cc, os.path.join(ROOT, "rtl-ws_amd", "csrc"), tmp_path_factory.mktemp("maps"), tile)


def test_the_kernels_build_their_tile_maps_as_the_host_check_does():
    for f in ("fm_chain.hip", "fm_bank.hip"):
        txt = open(os.path.join(ROOT, "rtl-ws_amd", "csrc", f)).read().replace("fm::", "")
        for line in fm_ref.TILE_MAP_TEXT:
            assert txt.count(line) == 1, (f, line)


def test_tile_map_equals_maps_in_the_product_text(host_maps):
    """fm_maps.h compiled for the host: for every block_len 20 .. 4200, over enough blocks for four tiles, TileMap as
    the kernels build it equals Maps at every position every tile reads, for both maps, and both equal fm_ref's numpy
    restatements; tile_range() equals fm_ref.tile_bounds."""
    print("tile %d: %d positions" % (host_maps.tile, fm_ref.sweep_host_maps(host_maps)))


@pytest.mark.parametrize("residue", [0, 1, 2, 3])
def test_tile_map_beyond_32_bits(host_maps, residue):
    """The 64/32-bit split: tiles whose stream positions lie on both sides of 2^31, 2^32 and 2^33 and at the end of
    a capture of more than 2^34 decimated samples, for tiny, tile-sized, long and the longest blocks."""
    fm_ref.check_host_maps_beyond_32_bits(host_maps, residue)


def test_wrong_tile_maps_pass_the_earlier_shapes_and_fail_the_new_ones(built):
    """The gap and its closure, on the CPU: a TileMap with dst0 counted in source blocks, one with src0 = 0 and one that
    maps nothing agree with Maps at every stage-1 position of every multi-tile launch the GPU suites made before, and
    disagree inside a tile of the new cases wherever block_len is not a multiple of 4."""
    fm_ref.check_wrong_tile_maps(built.fm_grid(20, 1, 0)[4])

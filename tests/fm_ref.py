"""Shared by the CPU and GPU suites of the FM chain and the FM bank: the oracle's per-block FM chain as a loop, the
test inputs, the kernels' stream maps (rtl-ws_amd/csrc/fm_maps.h: Maps, TileMap, tile_range) restated in numpy, the
block shapes of the multi-tile suites with the conditions they have to meet, and fm_maps.h compiled for the host."""
import numpy as np

STATE = 21


def oracle_chain(oracle, iq, block_len, state, run_stage2=True):
    """nblocks calls of oracle.audio_block (= audio_fm_demodulator) -> (audio, state out).  run_stage2=False is
    src/audio_main.c:137's exhausted pool: the second half-band never ran, its delay line keeps its value."""
    iq = np.ascontiguousarray(iq, dtype=np.int32).reshape(-1, 2)
    st = np.array(state, dtype=np.float32)
    out = []
    for b in range(iq.shape[0] // block_len):
        keep = st[11:21].copy()
        a = oracle.audio_block(iq[b * block_len:(b + 1) * block_len], st)
        if run_stage2:
            out.append(a)
        else:
            st[11:21] = keep
    audio = np.concatenate(out) if out else np.zeros(0, dtype=np.float32)
    return audio, st


def random_state(seed):
    """A non-zero carried state: a phase in (-pi, pi), delay lines of limiter-sized values."""
    rng = np.random.default_rng(seed)
    st = rng.uniform(-1.0, 1.0, STATE).astype(np.float32)
    st[0] = np.float32(rng.uniform(-3.0, 3.0))
    return st


def input_a(n, seed):
    """Random int32 in +-3000 with 1 % zeros in each component: the limiter and the x == 0 branches."""
    rng = np.random.default_rng(seed)
    iq = rng.integers(-3000, 3001, size=(n, 2), dtype=np.int32)
    iq[rng.random(n) < 0.01, 0] = 0
    iq[rng.random(n) < 0.01, 1] = 0
    return iq


def input_b(n, seed):
    """A phasor of amplitude 1000 with phase steps uniform in +-1.2 rad: both sides of the limiter."""
    rng = np.random.default_rng(seed)
    ph = np.cumsum(rng.uniform(-1.2, 1.2, n))
    return np.stack([np.round(1000 * np.cos(ph)), np.round(1000 * np.sin(ph))], axis=1).astype(np.int32)


# ---- the maps of fm_chain.hip ---------------------------------------------------------------------------------

def halfband_f32(x, hist):
    """Continuous 11-tap half-band over the stream x with hist = x[-10..-1]: float32, multiply then add, the
    centre tap first and the even taps in the order of src/resample.c:57-64."""
    h0, h2, h4, h5 = np.float32(0.01824), np.float32(-0.11614), np.float32(0.34790), np.float32(0.5)
    n = x.size // 2
    z = np.concatenate([np.asarray(hist, np.float32), np.asarray(x, np.float32)])
    c = 10 + 2 * np.arange(n)
    acc = h5 * z[c - 5]
    for h, k in ((h0, 0), (h2, 2), (h4, 4), (h4, 6), (h2, 8), (h0, 10)):
        acc = acc + h * z[c - k]
    assert acc.dtype == np.float32
    return acc


def s1_to_g(s1, L):
    half = L // 2
    return (s1 // (2 * half)) * L + s1 % (2 * half)


def s2_to_w(s2, L):
    half = L // 2
    quarter = half // 2
    return (s2 // (2 * quarter)) * half + s2 % (2 * quarter)


def chain_by_maps(oracle, iq, L, state):
    """The chain as ONE continuous filter over concatenated, truncated streams -> (audio, state out)."""
    iq = np.ascontiguousarray(iq, dtype=np.int32).reshape(-1, 2)
    nb = iq.shape[0] // L
    half = L // 2
    quarter = half // 2
    demod, last_phase = oracle.fm_demod(iq, prev_phase=float(state[0]))       # limit(phase[g] - phase[g-1])
    stage1 = demod[s1_to_g(np.arange(nb * 2 * half), L)]
    work = halfband_f32(stage1, state[1:11])
    stage2 = work[s2_to_w(np.arange(nb * 2 * quarter), L)]
    audio = halfband_f32(stage2, state[11:21])
    out = np.empty(STATE, dtype=np.float32)
    out[0] = np.float32(last_phase)
    out[1:11] = np.concatenate([state[1:11], stage1])[-10:]
    out[11:21] = np.concatenate([state[11:21], stage2])[-10:]
    return audio, out


def tile_bounds(t, L, nb, tile):
    """tile_range() of fm_maps.h, every field: what tile t of `tile` audio samples reads of each stream (bounds
    inclusive).  t, L and nb may be numpy int64 arrays."""
    quarter = (L // 2) // 2
    total = nb * quarter
    a0 = t * tile
    na = np.minimum(tile, total - a0)
    s2lo, s2hi = 2 * a0 - 10, 2 * (a0 + na - 1)
    wlo, whi = s2_to_w(np.maximum(s2lo, 0), L), s2_to_w(s2hi, L)
    s1lo = 2 * wlo - 10
    glo, ghi = s1_to_g(np.maximum(s1lo, 0), L), s1_to_g(2 * whi, L)
    return dict(a0=a0, na=na, s2lo=s2lo, wlo=wlo, whi=whi, s1lo=s1lo, glo=glo, ghi=ghi,
                n2=s2hi - s2lo + 1, n1=2 * (whi - wlo) + 11, np=ghi - glo + 2)


def tile_range(t, L, nb, tile):
    """tile_range() of fm_chain.hip: what tile t reads of each stream -> (n2, n1, np)."""
    r = tile_bounds(t, L, nb, tile)
    return int(r["n2"]), int(r["n1"]), int(r["np"])


class TileMap:
    """TileMap of fm_maps.h, constructor and operator(): the block that holds `from` by one 64-bit division, then the
    offset from that block's start as an unsigned 32-bit number.  Every argument may be an int64 array."""

    def __init__(self, from_, src_per_block, dst_per_block):
        self.n_src = np.asarray(src_per_block, dtype=np.int64)
        self.n_dst = np.asarray(dst_per_block, dtype=np.int64)
        b = np.asarray(from_, dtype=np.int64) // self.n_src
        self.src0 = b * self.n_src
        self.dst0 = b * self.n_dst

    def offset(self, s):
        return (np.asarray(s, dtype=np.int64) - self.src0) & 0xFFFFFFFF

    def __call__(self, s):
        s = np.asarray(s, dtype=np.int64)
        off = self.offset(s)
        b = off // self.n_src
        return np.where(self.n_src == self.n_dst, s, self.dst0 + b * self.n_dst + (off - b * self.n_src))


class _DstFromSrc(TileMap):
    def __init__(self, from_, src_per_block, dst_per_block):
        TileMap.__init__(self, from_, src_per_block, dst_per_block)
        self.dst0 = self.src0.copy()


class _SrcZero(TileMap):
    def __init__(self, from_, src_per_block, dst_per_block):
        TileMap.__init__(self, from_, src_per_block, dst_per_block)
        self.src0 = np.zeros_like(self.src0)


class _Identity(TileMap):
    def __call__(self, s):
        return np.asarray(s, dtype=np.int64)


# Three ways to get TileMap wrong that no launch over several tiles with a skipping stage-1 map would survive:
# dst0 counted in source blocks, the offset taken from position 0, no map at all.
WRONG_TILE_MAPS = {"dst0 from src_per_block": _DstFromSrc, "src0 = 0": _SrcZero, "identity": _Identity}


def stage_maps(L):
    """name -> (src_per_block, dst_per_block, the map of Maps) as the kernels build their two TileMaps."""
    half = L // 2
    return {"s1": (2 * half, L, s1_to_g), "s2": (2 * (half // 2), half, s2_to_w)}


def tile_reads(t, L, nb, tile):
    """name -> (from, positions): the positions tile t passes through each TileMap, and the `from` it is built on."""
    r = tile_bounds(t, L, nb, tile)
    out = {}
    for name, lo, n in (("s1", int(r["s1lo"]), int(r["n1"])), ("s2", int(r["s2lo"]), int(r["n2"]))):
        out[name] = (max(lo, 0), np.arange(max(lo, 0), lo + n, dtype=np.int64))
    return out


# ---- the block shapes of the multi-tile suites ------------------------------------------------------------------

class Case(tuple):
    """(regime, residue, block_len, nblocks)"""
    regime = property(lambda s: s[0])
    residue = property(lambda s: s[1])
    block_len = property(lambda s: s[2])
    nblocks = property(lambda s: s[3])
    id = property(lambda s: "%s%d-%dx%d" % s)

    def ntiles(self, tile):
        return -(-self.nblocks * (self.block_len // 4) // tile)


def tile_cases(tile):
    """The block shapes at which the two stream maps of a kernel with `tile` audio samples per workgroup are launched
    over several tiles, for every block_len mod 4 (1 and 3: the stage-1 map skips; 2 and 3: the stage-2 map skips):
      a  tiny blocks, block_len = 20 + r, dozens per tile (23 is the shape the LDS capacities are derived for): the
         fewest blocks whose audio is three tiles and a part of a fourth;
      b  quarter = tile - 2, four blocks: the borders lie 2, 4 and 6 audio samples in front of tiles 1, 2 and 3;
      c  block_len = 4100 + r: the fewest blocks, three at least, with three tiles and a part of one more and every
         border inside a tile.  Three, because a tile's map takes a block other than its first only when the tile
         begins behind the first border and holds the second."""
    cases = []
    for r in range(4):
        L = 20 + r
        nb = 3 * tile // (L // 4) + 1
        while nb * (L // 4) % tile == 0:
            nb += 1
        cases.append(Case(("a", r, L, nb)))
    for r in range(4):
        cases.append(Case(("b", r, 4 * (tile - 2) + r, 4)))
    for r in range(4):
        L = 4100 + r
        quarter = L // 4
        nb = max(3, -(-(3 * tile + 1) // quarter))
        while nb * quarter % tile == 0 or not all((b * quarter) % tile for b in range(1, nb)):
            nb += 1
        cases.append(Case(("c", r, L, nb)))
    return cases


def earlier_multi_tile_shapes(tile):
    """(block_len, nblocks) of every launch that the GPU suites made over more than one tile of either kernel before
    tile_cases(): tests/test_fm_gpu.py's 1024, 1030 and 4102 and tests/test_fmbank_gpu.py's 2 t + 6, 2 t + 8, t + 6, 1030, 4102."""
    nb = -(-(3 * tile + 1) // 1025)
    nb += (nb * 1025) % tile == 0
    return [(1024, 3), (1030, 3), (4102, 2), (4102, nb), (2 * tile + 6, 5), (2 * tile + 8, 5), (tile + 6, 5), (tile + 6, 3)]


def case_report(tile, worst):
    """Checks the conditions every tile_cases(tile) case has to meet, from the model alone, and returns the lines that
    say what the cases reach.  worst = the largest (n2, n1, np) over all block shapes, as the capacity tests find it."""
    lines = []
    for c in tile_cases(tile):
        regime, r, L, nb = c
        nt = c.ntiles(tile)
        assert nt >= 4 and nb * (L // 4) % tile != 0, c.id                  # four tiles at least, the last one partial
        fill = [max(x) for x in zip(*(tile_range(t, L, nb, tile) for t in range(nt)))]
        lines.append("tile %d, case %s: %d tiles, n2 <= %d, n1 <= %d, phases <= %d" % ((tile, c.id, nt) + tuple(fill)))
        for name, (n_src, n_dst, by_maps) in stage_maps(L).items():
            skips = {"s1": r in (1, 3), "s2": r in (2, 3)}[name]
            assert (n_src != n_dst) == skips, (c.id, name)
            if not skips:
                continue
            later_block = []
            for t in range(1, nt):
                from_, pos = tile_reads(t, L, nb, tile)[name]
                m = TileMap(from_, n_src, n_dst)
                assert np.array_equal(m(pos), by_maps(pos, L)), (c.id, name, t)
                if m.src0 > 0 and (m.offset(pos) // n_src).max() >= 1:
                    later_block.append(t)
            assert later_block, (c.id, name)
        if regime == "b":
            half = L // 2
            halo = lambda lo, per_block: any(s > 0 and s % per_block == 0 for s in range(lo, lo + 10))
            for t in (1, 2):
                assert halo(int(tile_bounds(t, L, nb, tile)["s2lo"]), 2 * (half // 2)), (c.id, t)
            assert halo(int(tile_bounds(3, L, nb, tile)["s1lo"]), 2 * half), c.id
        if L == 23:
            assert fill == list(worst), (fill, worst)
            lines.append("tile %d, block_len 23: the launch fills as far as any shape can" % tile)
    return lines


# ---- fm_maps.h compiled for the host ----------------------------------------------------------------------------

_HOST_SRC = r"""
#include "fm_maps.h"
using namespace rtlws::fm;
// every position the given tiles pass through their two TileMaps, built as the kernels build them
extern "C" long walk(int L, long nblocks, const long* tiles, int ntiles, long cap, long* which, long* pos, long* from_,
                     long* by_maps, long* by_tile)
{
    const Maps m = make_maps(L, nblocks);
    long n = 0;
    for (int i = 0; i < ntiles; ++i) {
        const TileRange r = tile_range<HOST_TILE>(m, tiles[i]);
        const TileMap to_g(r.s1lo < 0 ? 0 : r.s1lo, m.L1, m.L);
        const TileMap to_w(r.s2lo < 0 ? 0 : r.s2lo, m.L2, m.half);
        for (int j = 0; j < r.n1; ++j) {
            const long s1 = r.s1lo + j;
            if (s1 < 0) continue;
            if (n == cap) return -1;
            which[n] = 1, pos[n] = s1, from_[n] = r.s1lo < 0 ? 0 : r.s1lo, by_maps[n] = m.s1_to_g(s1), by_tile[n++] = to_g(s1);
        }
        for (int j = 0; j < r.n2; ++j) {
            const long s2 = r.s2lo + j;
            if (s2 < 0) continue;
            if (n == cap) return -1;
            which[n] = 2, pos[n] = s2, from_[n] = r.s2lo < 0 ? 0 : r.s2lo, by_maps[n] = m.s2_to_w(s2), by_tile[n++] = to_w(s2);
        }
    }
    return n;
}
extern "C" void range(int L, long nblocks, long t, long* out)
{
    const TileRange r = tile_range<HOST_TILE>(make_maps(L, nblocks), t);
    const long v[11] = {r.a0, r.na, r.s2lo, r.wlo, r.whi, r.s1lo, r.glo, r.ghi, r.n2, r.n1, r.np};
    for (int i = 0; i < 11; ++i) out[i] = v[i];
}
"""
RANGE_FIELDS = ("a0", "na", "s2lo", "wlo", "whi", "s1lo", "glo", "ghi", "n2", "n1", "np")
# how the kernels build their TileMaps: _HOST_SRC builds them with the same text
TILE_MAP_TEXT = ("const TileMap to_g(r.s1lo < 0 ? 0 : r.s1lo, m.L1, m.L);", "const TileMap to_w(r.s2lo < 0 ? 0 : r.s2lo, m.L2, m.half);")


class HostMaps:
    """rtl-ws_amd/csrc/fm_maps.h as it stands, compiled by the host's C++ compiler for a tile of `tile` audio samples:
    an empty <hip/hip_runtime.h> in front of the include path and the two qualifiers defined away."""

    def __init__(self, compiler, csrc, tmp_path, tile):
        import ctypes
        import subprocess
        (tmp_path / "hip").mkdir(exist_ok=True)
        (tmp_path / "hip" / "hip_runtime.h").write_text("")
        src = tmp_path / ("maps_%d.cpp" % tile)
        src.write_text(_HOST_SRC)
        so = tmp_path / ("maps_%d.so" % tile)
        subprocess.run([compiler, "-O2", "-std=c++17", "-shared", "-fPIC", "-D__device__=", "-D__forceinline__=inline",
                        "-DHOST_TILE=%d" % tile, "-I", str(tmp_path), "-I", csrc, str(src), "-o", str(so)], check=True)
        self.lib = ctypes.CDLL(str(so))
        p = ctypes.c_void_p
        self.lib.walk.restype = ctypes.c_long
        self.lib.walk.argtypes = [ctypes.c_int, ctypes.c_long, p, ctypes.c_int, ctypes.c_long, p, p, p, p, p]
        self.lib.range.restype = None
        self.lib.range.argtypes = [ctypes.c_int, ctypes.c_long, ctypes.c_long, p]
        self.tile = tile

    def walk(self, L, nb, tiles):
        """-> int64 arrays (which map: 1 or 2, position, the map's `from`, by Maps, by TileMap)"""
        tiles = np.ascontiguousarray(tiles, dtype=np.int64)
        cap = tiles.size * (8 * self.tile + 64)
        out = np.empty((5, cap), dtype=np.int64)
        n = self.lib.walk(L, nb, tiles.ctypes.data, tiles.size, cap, *[out[i].ctypes.data for i in range(5)])
        assert n >= 0, "more positions than a tile can read"
        return out[:, :n]

    def range(self, L, nb, t):
        out = np.empty(11, dtype=np.int64)
        self.lib.range(L, nb, t, out.ctypes.data)
        return dict(zip(RANGE_FIELDS, (int(v) for v in out)))


def host_compiler():
    import shutil
    for c in ("g++", "c++", "clang++"):
        if shutil.which(c):
            return c
    return None


def check_host_maps(host, L, nb, tiles):
    """TileMap and Maps of the product text and the numpy maps agree at every position the tiles read -> positions"""
    which, pos, from_, by_maps, by_tile = host.walk(L, nb, tiles)
    bad = np.nonzero(by_maps != by_tile)[0]
    assert bad.size == 0, (L, nb, which[bad[:4]], pos[bad[:4]], by_maps[bad[:4]], by_tile[bad[:4]])
    for k, name in ((1, "s1"), (2, "s2")):
        n_src, n_dst, numpy_map = stage_maps(L)[name]
        sel = which == k
        assert np.array_equal(numpy_map(pos[sel], L), by_maps[sel]), (L, nb, name)
        assert np.array_equal(TileMap(from_[sel], n_src, n_dst)(pos[sel]), by_tile[sel]), (L, nb, name)
    return which.size


def case_input(make, case):
    """(iq, carried state) of a case for the cs32 chain; make = input_a or input_b"""
    seed = 100 * case.block_len + case.nblocks
    return make(case.block_len * case.nblocks, seed=seed), random_state(seed + 1)


def check_wrong_tile_maps(tile):
    for name, wrong in WRONG_TILE_MAPS.items():
        for L, nb in earlier_multi_tile_shapes(tile):
            n_src, n_dst, by_maps = stage_maps(L)["s1"]
            for t in range(-(-nb * (L // 4) // tile)):
                from_, pos = tile_reads(t, L, nb, tile)["s1"]
                assert np.array_equal(wrong(from_, n_src, n_dst)(pos), by_maps(pos, L)), (name, L, t)
        for c in tile_cases(tile):
            if c.residue == 0:
                continue
            caught = []
            for t in range(c.ntiles(tile)):
                for stream, (from_, pos) in tile_reads(t, c.block_len, c.nblocks, tile).items():
                    n_src, n_dst, by_maps = stage_maps(c.block_len)[stream]
                    if not np.array_equal(wrong(from_, n_src, n_dst)(pos), by_maps(pos, c.block_len)):
                        caught.append((t, stream))
            assert caught, (name, c.id)
            if c.residue in (1, 3):
                assert any(t >= 1 and stream == "s1" for t, stream in caught), (name, c.id)


def sweep_host_maps(host):
    """every block_len 20 .. 4200, every tile of enough blocks for four tiles -> positions checked"""
    tile, n = host.tile, 0
    for L in range(20, 4201):
        quarter = L // 4
        nb = -(-4 * tile // quarter) + 1
        ntiles = -(-nb * quarter // tile)
        assert ntiles >= 4
        n += check_host_maps(host, L, nb, np.arange(ntiles))
        for t in (0, ntiles // 2, ntiles - 1):
            want = tile_bounds(t, L, nb, tile)
            assert host.range(L, nb, t) == {k: int(want[k]) for k in RANGE_FIELDS}, (L, t)
    return n


def check_host_maps_beyond_32_bits(host, residue):
    """Tiles whose positions lie on both sides of 2^31, 2^32 and 2^33 and at the end of a capture of more than 2^34
    decimated samples, for tiny, tile-sized, long and the longest blocks of one residue of block_len mod 4."""
    tile = host.tile
    for L in (20 + residue, 4 * (tile - 2) + residue, 4100 + residue, (1 << 24) - 4 + residue):
        quarter = L // 4
        nb = (1 << 34) // L + 3
        ntiles = -(-nb * quarter // tile)
        tiles = {ntiles - 1, ntiles - 2, ntiles - 3}
        for edge in (1 << 31, 1 << 32, 1 << 33):
            for per_audio in (1, 2, 4, 5):              # audio, stage 2, stage 1, samples (up to 23 for 5 audio samples)
                t = edge // (per_audio * tile)
                tiles |= {t - 1, t, t + 1}
        tiles = np.array(sorted(t for t in tiles if 0 <= t < ntiles))
        _, pos, from_, by_maps, _ = host.walk(L, nb, tiles)
        assert pos.max() > 1 << 33 and from_.max() > 1 << 33 and by_maps.max() >= (1 << 34) - 1
        check_host_maps(host, L, nb, tiles)

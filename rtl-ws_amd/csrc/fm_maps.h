// fm_maps.h -- the stream maps of the FM receive chain (tests/fm_ref.py restates them in numpy), one
// text of each: a block of L decimated samples keeps 2 half of them for the first half-band and 2 quarter of its
// outputs for the second, and a tile of audio samples walks those two maps back to the samples it needs.  Shared by
// the chain of one stream (fm_chain.hip) and the chain behind the down-converter bank (fm_bank.hip).
#ifndef RTLWS_FM_MAPS_H
#define RTLWS_FM_MAPS_H

#include <hip/hip_runtime.h>

namespace rtlws {
namespace fm {

// the two index maps, stream position -> position in the stream it is cut from
struct Maps {
    int L, half, L1, L2;      // L1 = 2 half, L2 = 2 quarter
    long nblocks;
    __device__ long s2_to_w(long s2) const
    {
        if (L2 == half) return s2;
        const long b = s2 / L2;
        return b * half + (s2 - b * L2);
    }
    __device__ long s1_to_g(long s1) const
    {
        if (L1 == L) return s1;
        const long b = s1 / L1;
        return b * L + (s1 - b * L1);
    }
};

// The same map for positions at or after `from`, with the one 64-bit division done once per workgroup: a tile spans
// fewer than 2^12 positions and a block fewer than 2^31, so the offset from the block that holds `from` fits 32 bits.
struct TileMap {
    long src0, dst0;
    unsigned n_src, n_dst;
    __device__ TileMap(long from, int src_per_block, int dst_per_block)
        : n_src((unsigned)src_per_block), n_dst((unsigned)dst_per_block)
    {
        const long b = from / src_per_block;
        src0 = b * src_per_block;
        dst0 = b * dst_per_block;
    }
    __device__ long operator()(long s) const
    {
        if (n_src == n_dst) return s;
        const unsigned off = (unsigned)(s - src0);
        const unsigned b = off / n_src;
        return dst0 + (long)b * n_dst + (off - b * n_src);
    }
};

__device__ __forceinline__ Maps make_maps(int block_len, long nblocks)
{
    Maps m;
    m.L = block_len;
    m.half = m.L / 2;
    m.L1 = 2 * m.half;
    m.L2 = 2 * (m.half / 2);
    m.nblocks = nblocks;
    return m;
}

// what tile t needs of every stream (all bounds inclusive)
struct TileRange {
    long a0, s2lo, wlo, whi, s1lo, glo, ghi;
    int na, n2, n1, np;
};

// tile t of TILE_AUDIO consecutive audio samples
template <int TILE_AUDIO>
__device__ __forceinline__ TileRange tile_range(const Maps& m, long t)
{
    TileRange r;
    const long total_audio = m.nblocks * (m.L2 / 2);
    r.a0 = t * TILE_AUDIO;
    r.na = (int)(total_audio - r.a0 < TILE_AUDIO ? total_audio - r.a0 : TILE_AUDIO);
    r.s2lo = 2 * r.a0 - 10;                              // the delay line of the first output
    const long s2hi = 2 * (r.a0 + r.na - 1);
    r.n2 = (int)(s2hi - r.s2lo) + 1;
    r.wlo = m.s2_to_w(r.s2lo < 0 ? 0 : r.s2lo);
    r.whi = m.s2_to_w(s2hi);
    r.s1lo = 2 * r.wlo - 10;
    r.n1 = 2 * (int)(r.whi - r.wlo) + 11;
    r.glo = m.s1_to_g(r.s1lo < 0 ? 0 : r.s1lo);
    r.ghi = m.s1_to_g(2 * r.whi);
    r.np = (int)(r.ghi - r.glo) + 2;                     // phases glo - 1 .. ghi
    return r;
}

}  // namespace fm
}  // namespace rtlws
#endif

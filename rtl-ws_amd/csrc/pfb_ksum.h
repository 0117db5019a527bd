// pfb_ksum.h -- what the kernels that sum K frames over the polyphase filter bank's tile share (pfbspec.hip,
// pfbxc.hip, pfbbf.hip): the power of a bin and the passes' call inside a loop.  The geometry
// of the sums is pfb_bank.h's.  Their order,
//
//   S = ((A_0 + A_1) + ..) + A_(n-1),  A_s = (((+0 + P[s SLICE]) + P[s SLICE + 1]) + ..)     SLICE = slice_frames(K)
//
// which rtlws_pfbxc.h and rtlws_pfbbf.h promise to be the spectrometer's bit for bit, stays spelled out in each
// kernel: one text of the slice loop, of the combine through LDS and of the (spectrum, bin) loop compiled to other
// instructions in every kernel that took it, and rows of all three libraries then measured outside the spread of
// the kernels' own text (profiles/pfb_family_refactor_ab.txt).  tests/test_pfb*_gpu.py hold the three to one order;
// tests/test_pfb_ksum_gpu.py holds it to the bit at a K of every class of (log2 M, K) (tests/pfb_ksum_cases.py).
#ifndef RTLWS_PFB_KSUM_H
#define RTLWS_PFB_KSUM_H

#include "pfb_tile.h"

namespace rtlws {
namespace pfb {

// fl(fl(re re) + fl(im im)): the products pass through an empty asm, so the sum cannot take one of them into a
// fused multiply-add (the files are compiled with contraction on, as the filter bank's transform needs)
__device__ __forceinline__ float power(float2 y)
{
    float a = y.x * y.x, b = y.y * y.y;
    asm("" : "+v"(a));
    asm("" : "+v"(b));
    return a + b;
}

// Passes 1 .. 4 (pfb_tile.h) inside a loop over tile iterations or captures.  The thread index and the arrays'
// addresses are made opaque before every call: what the passes derive from them (some forty addresses and the first
// loads) is formed inside the loop, as in the channelizer's kernel, and not held in registers across it, which would
// cost a workgroup per compute unit.  Returns the opaque thread index.
template <int K>
__device__ __forceinline__ int tile_passes_afresh(PfbParams& bank, long m0, int tid, float2* tile)
{
    int t = tid;
    asm volatile("" : "+v"(t), "+s"(bank.src), "+s"(bank.taps), "+s"(bank.tw));
    tile_passes<K>(bank, m0, t, tile);
    return t;
}

}  // namespace pfb
}  // namespace rtlws
#endif

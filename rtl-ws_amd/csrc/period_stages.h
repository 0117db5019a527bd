// period_stages.h -- what the kernels of the periodicity-search family take from one text behind the transform
// (DESIGN.md 4.22, 4.24a): the rule by which two partial peaks meet, over two values and over the lanes of a wavefront,
// the real-input untangling of one pair of bins and the square.  period.hip and periodlong.hip (and with it the
// acceleration search) include it.  The whitening and the harmonic walk stay written out in both kernels' files: as
// __forceinline__ templates they compile to other instructions than the text in place.
#ifndef RTLWS_CSRC_PERIOD_STAGES_H
#define RTLWS_CSRC_PERIOD_STAGES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs.h"
#include "period.h"

namespace rtlws {
namespace period {
namespace stages {

// the rule of the peaks between two partial results (best, at): the strict maximum, ties to the smaller k; a partial
// that took nothing is (-Inf, -1) and never wins
__device__ __forceinline__ void meet(float& best, int& at, float ob, int oa)
{
    if (ob > best || (ob == best && oa < at)) best = ob, at = oa;
}

__device__ __forceinline__ void meet_lanes(float& best, int& at)
{
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) {
        const float ob = __shfl_xor(best, off);
        const int oa = __shfl_xor(at, off);
        meet(best, at, ob, oa);
    }
}

// The real-input untangling of one pair: X[k] = E - i W^k O, X[M - k] = conj(E) - i conj(W^k O),
// E, O = (Z[k] +- conj Z[M - k]) / 2; za = Z[k], zb = Z[M - k], w = W^k -> a = X[k], b = X[M - k].  The bin that is its own
// mirror passes zb = za and takes a alone
struct Pair {
    f2 a, b;
};

__device__ __forceinline__ Pair untangle(f2 za, f2 zb, float2 w)
{
    const f2 e = mk(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));
    const f2 o = mk(0.5f * (za.x - zb.x), 0.5f * (za.y + zb.y));
    const f2 t = cmul(o, mk(w.x, w.y));
    return Pair{mk(e.x + t.y, e.y - t.x), mk(e.x - t.y, e.y + t.x)};
}

// the power of a bin, one fused rounding behind the product
__device__ __forceinline__ float power(f2 x) { return fmaf(x.x, x.x, x.y * x.y); }

}  // namespace stages
}  // namespace period
}  // namespace rtlws
#endif

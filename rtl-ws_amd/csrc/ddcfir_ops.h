// ddcfir_ops.h -- the two pieces of the filtered down-converter's contraction that more than one kernel compiles
// (include/rtlws_ddcfir.h), one text of each: the int8 A operands of the taps times the channel's
// phasors, and the loader of a window's B operand.  Shared by the bank that stores the filtered samples
// (ddcfir_bank.hip) and the bank that demodulates them in place (fmfir_bank.hip); the operand and lane maps are
// described at the head of ddcfir_bank.hip, the byte split and the rotation are ddc_ops.h's.
#ifndef RTLWS_DDCFIR_OPS_H
#define RTLWS_DDCFIR_OPS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_ops.h"
#include "ddcfir.h"

namespace rtlws {
namespace ddcfir {

// The A operands of lane `lane` for column tile ct and K step ks: {high bytes (2 dwords), low bytes (2 dwords)} of
// G of taps n = 16 ks + 4 (lane >> 4) + t, t < 4, on row lane & 15.  Zero beyond L and beyond C.
// Params has .table, .taps, .words, .nch and .ntaps (FirParams, fmfir::BankParams).
template <class Params>
__device__ __forceinline__ uint4 filter_operand(const Params& p, int ct, int ks, int lane)
{
    const int r = lane & 15, q = lane >> 4;
    const int c = 8 * ct + (r >> 1);
    const bool im_row = r & 1;
    const int k = p.words[c & (MAX_CH - 1)];
    unsigned hi[2] = {0u, 0u}, lo[2] = {0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int n = 16 * ks + 4 * q + t;
        int w_re = 0, w_im = 0;                          // what multiplies the sample's re byte and its im byte
        if (c < p.nch && n < p.ntaps) {
            const int2 e = ddc::phasor(p.table, (unsigned)(k * n));
            const int h = p.taps[n];
            const int gc = (h * e.x + (1 << 13)) >> 14, gs = (h * e.y + (1 << 13)) >> 14;
            w_re = im_row ? -gs : gc;
            w_im = im_row ? gc : gs;
        }
        ddc::split_bytes(hi, lo, t, w_re, w_im);
    }
    return make_uint4(hi[0], hi[1], lo[0], lo[1]);
}

// Samples n0 .. n0 + 3 of the window of decimated sample m, two bytes each; nothing from sample L on is read (zero
// there).  The windows are re-read by the neighbouring outputs: plain loads, the caches keep them.
template <bool ALIGNED>
__device__ __forceinline__ long load_window(const void* src, long m, int R, int L, int n0)
{
    if constexpr (ALIGNED) {                             // R, L, n0 multiples of four: all four samples or none
        if (n0 >= L) return 0;
        const ddc::nt_u2 v = *reinterpret_cast<const ddc::nt_u2*>(reinterpret_cast<const uint16_t*>(src) + m * R + n0);
        return ddc::pack(v.x, v.y);
    } else {
        const uint16_t* s = reinterpret_cast<const uint16_t*>(src) + m * R;
        if (((R | L) & 1) == 0) {                        // both even (the same for every lane): whole pairs, 4-byte aligned
            const unsigned lo = n0 < L ? *reinterpret_cast<const unsigned*>(s + n0) : 0u;
            const unsigned hi = n0 + 2 < L ? *reinterpret_cast<const unsigned*>(s + n0 + 2) : 0u;
            return ddc::pack(lo, hi);
        }
        unsigned v[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) v[t] = n0 + t < L ? (unsigned)s[n0 + t] : 0u;
        return ddc::pack(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
    }
}

}  // namespace ddcfir
}  // namespace rtlws
#endif

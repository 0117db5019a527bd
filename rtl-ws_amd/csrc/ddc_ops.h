// ddc_ops.h -- the integer pieces of the down-converter's decimated sample (include/rtlws_ddc.h), one
// text of each: the phasor lookup, the int8 A operands of v_mfma_i32_16x16x32_i8 and their byte split, the loaders of
// the B operand, the block-phasor rotation and the store of a lane's two channels.  Shared by the bank that stores the
// samples (ddc_bank.hip), the bank that demodulates them in place (fm_bank.hip) and the bank that filters them
// (ddcfir_bank.hip: the byte split, the rotation, the store); the operand and lane maps are described at the head of
// ddc_bank.hip; DESIGN.md 4.13b says what stayed per kernel.
#ifndef RTLWS_DDC_OPS_H
#define RTLWS_DDC_OPS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_bank.h"

namespace rtlws {
namespace ddc {

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int nt_i2 __attribute__((ext_vector_type(2)));
typedef unsigned nt_u2 __attribute__((ext_vector_type(2)));

// T[phase mod P] as (cos, sin)
__device__ __forceinline__ int2 phasor(const uint32_t* __restrict__ table, unsigned phase)
{
    const uint32_t e = table[phase & (unsigned)(P - 1)];
    return make_int2((int)(int16_t)(e & 0xffffu), (int)e >> 16);
}

// An int16 w as two int8 operands, w = 256 wh + wl with wl in -128 .. 127: the pair (w_re, w_im) that multiplies the re
// and the im byte of sample t (of a lane's four) goes into the high-byte and the low-byte dwords at that sample
__device__ __forceinline__ void split_bytes(unsigned (&hi)[2], unsigned (&lo)[2], int t, int w_re, int w_im)
{
    const int re_l = (int8_t)w_re, im_l = (int8_t)w_im;
    const unsigned pair_l = ((unsigned)re_l & 0xffu) | (((unsigned)im_l & 0xffu) << 8);
    const unsigned pair_h = ((unsigned)((w_re - re_l) >> 8) & 0xffu) | (((unsigned)((w_im - im_l) >> 8) & 0xffu) << 8);
    lo[t >> 1] |= pair_l << (16 * (t & 1));
    hi[t >> 1] |= pair_h << (16 * (t & 1));
}

// The A operands of lane `lane` for column tile ct and K step ks: {high bytes (2 dwords), low bytes (2 dwords)}
// of the phasors of samples n = 16 ks + 4 (lane >> 4) + t, t < 4, on row lane & 15.  Zero beyond R and beyond C.
// Params has .table, .words, .nch and .cic_r (BankParams, fmbank::BankParams).
template <class Params>
__device__ __forceinline__ uint4 phasor_operand(const Params& p, int ct, int ks, int lane)
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
        if (c < p.nch && n < p.cic_r) {
            const int2 e = phasor(p.table, (unsigned)(k * n));
            w_re = im_row ? -e.y : e.x;
            w_im = im_row ? e.x : e.y;
        }
        split_bytes(hi, lo, t, w_re, w_im);
    }
    return make_uint4(hi[0], hi[1], lo[0], lo[1]);
}

__device__ __forceinline__ long pack(unsigned lo, unsigned hi) { return (long)(((unsigned long)hi << 32) | lo); }

// Bytes 8 q .. 8 q + 7 of the block of decimated sample m (zero behind the block).  Streamed once: nontemporal.
template <int RT>
__device__ __forceinline__ long load_block(const void* src, long m, int q)
{
    if constexpr (RT == 8) {                             // 16 bytes: two lanes of eight
        if (q >= 2) return 0;
        const nt_u2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u2*>(src) + m * 2 + q);
        return pack(v.x, v.y);
    } else if constexpr (RT == 12) {                     // 24 bytes, 8-byte aligned: three lanes of eight
        if (q >= 3) return 0;
        const nt_u2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_u2*>(src) + m * 3 + q);
        return pack(v.x, v.y);
    } else {                                             // R = 10: 20 bytes, 4-byte aligned: dwords 2 q, 2 q + 1 of five
        static_assert(RT == 10, "compile-time factors: 8, 10, 12");
        if (q >= 3) return 0;
        const unsigned* w = reinterpret_cast<const unsigned*>(src) + m * 5 + 2 * q;
        const unsigned lo = __builtin_nontemporal_load(w);
        const unsigned hi = q < 2 ? __builtin_nontemporal_load(w + 1) : 0u;
        return pack(lo, hi);
    }
}

// any factor: samples n0 .. n0 + 3 of the block of decimated sample m, two bytes each (zero from sample R on)
__device__ __forceinline__ long load_any(const void* src, long m, int R, int n0)
{
    const uint16_t* s = reinterpret_cast<const uint16_t*>(src) + m * R;
    unsigned v[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) v[t] = n0 + t < R ? (unsigned)s[n0 + t] : 0u;
    return pack(v[0] | (v[1] << 16), v[2] | (v[3] << 16));
}

// One component of the inner sum from its two accumulators: 256 (A_h B) + A_l B
__device__ __forceinline__ int inner_sum(int hi, int lo) { return (int)(((unsigned)hi << 8) + (unsigned)lo); }

// (U * conj(e) + 2^(13 + s) (1 + i)) >> (14 + s) with e the block phasor: int64, arithmetic shift
__device__ __forceinline__ int2 rotate_shift(int ur, int ui, int2 e, int s)
{
    const long r = 1L << (13 + s);
    const long vr = (long)ur * e.x + (long)ui * e.y + r;
    const long vi = (long)ui * e.x - (long)ur * e.y + r;
    return make_int2((int)(vr >> (14 + s)), (int)(vi >> (14 + s)));
}

// the unfiltered banks' rotation: (U * conj(e) + 2^27 (1 + i)) >> 28
constexpr int SHIFT = 14;
__device__ __forceinline__ int2 rotate(int ur, int ui, int2 e) { return rotate_shift(ur, ui, e, SHIFT); }

// the rotation's shift s of a bank: the unfiltered one's is fixed, ddcfir::FirParams brings the caller's (ddcfir.h)
__device__ __forceinline__ constexpr int shift_of(const BankParams&) { return SHIFT; }

// The block phasor and the store: this lane's two channels c0, c0 + 1 of decimated sample m.
// Params has .out, .out_stride, .table, .first, .nch and a shift_of (BankParams, ddcfir::FirParams).
template <class Params>
__device__ __forceinline__ void emit(const Params& p, v4i hi, v4i lo, int c0, unsigned kr0, unsigned kr1, long m)
{
    const unsigned g16 = ((unsigned)p.first + (unsigned)m) & 0xffffu;      // only the low 16 bits of k R g matter
    nt_i2* out = reinterpret_cast<nt_i2*>(p.out);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (c0 + h >= p.nch) continue;
        const int2 v = rotate_shift(inner_sum(hi[2 * h], lo[2 * h]), inner_sum(hi[2 * h + 1], lo[2 * h + 1]),
                                    phasor(p.table, (h ? kr1 : kr0) * g16), shift_of(p));
        const nt_i2 o = {v.x, v.y};
        out[(long)(c0 + h) * p.out_stride + m] = o;
    }
}

}  // namespace ddc
}  // namespace rtlws
#endif

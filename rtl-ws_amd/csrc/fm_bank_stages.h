// fm_bank_stages.h -- what an FM bank's workgroup does around its stage A, one text of each piece (DESIGN.md 4.13,
// 4.13c): the LDS arrays of a channel, the range of the workgroup behind the last tile, a lane's two phases out of the
// contraction's accumulators, one output of the first half-band, and the state copy of a call without blocks.  Shared
// by the bank over the CIC block sum (fm_bank.hip) and the bank over an int16 FIR (fmfir_bank.hip).  Stages B - D and
// the writer of state_out are each kernel's own text: as shared functions they gave fm_bank_kernel other instructions
// (DESIGN.md 4.13c says which form and what differed).  Params has .state_in, .nch and a shift_of
// (fmbank::BankParams, fmfir::BankParams).  Units that include this are built with -ffp-contract=off.
#ifndef RTLWS_FM_BANK_STAGES_H
#define RTLWS_FM_BANK_STAGES_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_ops.h"
#include "fm_bank.h"
#include "fm_maps.h"
#include "fm_math.h"

namespace rtlws {
namespace fmbank {

using ddc::v4i;

__device__ __forceinline__ float* phase_of_ch(float* lds, int ch) { return lds + ch * PHASE_CAP; }
__device__ __forceinline__ float* s1_of_ch(float* lds, int ch) { return lds + COL_CH * PHASE_CAP + ch * S1_CAP; }

// the shift s of the rotation in front of the discriminator: the unfiltered bank's is ddc_ops.h's fixed one,
// fmfir::BankParams brings the caller's (fmfir.h)
__device__ __forceinline__ constexpr int shift_of(const BankParams&) { return ddc::SHIFT; }

// What the workgroup behind the last tile needs: the last ten positions of the stage-2 stream (all in the last
// block: 2 quarter >= 10), the stage-1 stream from the delay line of the first of them to its end, the samples
// under that to the last one.  At most 34 stage-1 positions and 40 phases.
__device__ __forceinline__ fm::TileRange tail_range(const fm::Maps& m)
{
    fm::TileRange r;
    const long n2_all = m.nblocks * m.L2, n1_all = m.nblocks * m.L1;
    r.a0 = 0;
    r.na = 0;
    r.s2lo = n2_all - 10;
    r.n2 = 10;
    r.wlo = m.s2_to_w(r.s2lo);
    r.whi = m.s2_to_w(n2_all - 1);
    r.s1lo = 2 * r.wlo - 10;
    r.n1 = (int)(n1_all - r.s1lo);
    r.glo = m.s1_to_g(r.s1lo < 0 ? 0 : r.s1lo);
    r.ghi = m.nblocks * m.L - 1;
    r.np = (int)(r.ghi - r.glo) + 2;
    return r;
}

// This lane's two channels c0, c0 + 1 of decimated sample g, phase index idx: the block phasor (its table entry e),
// the conversion, the phase.  Sample -1 is the carried phase.
template <class Params>
__device__ __forceinline__ void emit_phase(const Params& p, float* ph, v4i hi, v4i lo, int c0, const uint32_t (&e)[2], long g,
                                           int idx)
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        if (c0 + h >= p.nch) continue;
        float v;
        if (g < 0) {
            v = p.state_in[(c0 + h) * STATE];
        } else {
            const int2 ph_blk = make_int2((int)(int16_t)(e[h] & 0xffffu), (int)e[h] >> 16);
            const int2 s = ddc::rotate_shift(ddc::inner_sum(hi[2 * h], lo[2 * h]), ddc::inner_sum(hi[2 * h + 1], lo[2 * h + 1]),
                                             ph_blk, shift_of(p));
            v = atan2_approx_dev((float)s.y, (float)s.x);
        }
        ph[h * PHASE_CAP + idx] = v;
    }
}

// One output of the first half-band from a channel's stage-1 arrays: output w sits at stage-1 position
// 2 w = s1lo + 2 k with k = w - wlo + 5 (fm_chain.hip, stage C)
__device__ __forceinline__ float work_at(const float* s1e, int k)
{
    const float* s1o = s1e + S1_HALF;
    return halfband_dev(s1o[k - 3], s1e[k], s1e[k - 1], s1e[k - 2], s1e[k - 3], s1e[k - 4], s1e[k - 5]);
}

__global__ __launch_bounds__(THREADS) void fm_bank_state_copy_kernel(const float* __restrict__ in, float* __restrict__ out,
                                                                      int nfloats)
{
    for (int i = threadIdx.x; i < nfloats; i += THREADS) out[i] = in[i];
}

}  // namespace fmbank
}  // namespace rtlws
#endif

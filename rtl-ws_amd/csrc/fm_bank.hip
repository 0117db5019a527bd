// fm_bank.hip -- up to 32 FM stations from one cmplx_u8 capture as ONE kernel (include/rtlws_fmbank.h): the decimated
// samples of the down-converter bank (ddc_bank.hip) are demodulated where they are formed, and the chain of
// fm_chain.hip runs per channel out of LDS.  2 * cic_r bytes in per decimated sample and one byte out per channel and
// decimated sample; nothing in between touches device memory.  Built with -ffp-contract=off.
//
// A workgroup owns TILE consecutive audio samples of one column tile of eight channels.  It walks fm_chain.hip's two
// index maps (fm_maps.h) back to the decimated samples glo - 1 .. ghi and forms them, sixteen at a time per
// wavefront, with ddc_bank.hip's contraction (ddc_ops.h: the same operands, the same lane map, the same rotation --
// the integers are rtlws_ddc_run's).  In the accumulator's lane map a lane holds (re, im) of two channels of one
// sample: the conversion to f32 and atan2_approx follow on that lane, and the phase goes to the channel's array in
// LDS.  Stages B - D are fm_chain.hip's, with the index arithmetic of a stream position done once for the eight
// channels.  Per column tile one more workgroup, the last, does the same for the few samples behind the tails of the
// three streams and writes state_out; state_in and state_out differ, so there is no ordering between workgroups.
// The pieces that fmfir_bank.hip compiles too are fm_bank_stages.h's.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_ops.h"
#include "fm_bank.h"
#include "fm_bank_stages.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace fmbank {

constexpr int GROUP = 4;                  // row tiles of a wavefront whose loads are in flight together

// A. the phases of decimated samples glo - 1 .. glo - 2 + np of the column tile's channels into LDS.
// RT = 8, 10, 12: that factor, one K step, the phasor operands in registers.  RT = 0: any factor 1 .. 128, the
// operands in LDS over the stage-1 streams (which the caller fills after its barrier).
template <int RT>
__device__ __forceinline__ void phases(const BankParams& p, int ct, long glo, int np, float* lds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int R = RT ? RT : p.cic_r;
    const int c0 = COL_CH * ct + 2 * q;
    const int nrt = (np + ddc::ROWS - 1) / ddc::ROWS;
    float* ph = phase_of_ch(lds, 2 * q);
    unsigned kr[2];                                      // k_c R mod P of the channels this lane holds
#pragma unroll
    for (int h = 0; h < 2; ++h) kr[h] = (unsigned)(p.words[(c0 + h) & (MAX_CH - 1)] * R) & 0xffffu;
    const v4i zero = {0, 0, 0, 0};

    if constexpr (RT != 0) {
        const uint4 a = ddc::phasor_operand(p, ct, 0, lane);
#pragma unroll 1
        for (int rt0 = wave * GROUP; rt0 < nrt; rt0 += WAVES * GROUP) {
            long b[GROUP];                               // every load and every block-phasor lookup of the group in flight
            uint32_t e[GROUP][2];
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const int idx = (rt0 + i) * ddc::ROWS + j;
                const long g = glo - 1 + idx;
                const bool ok = idx < np && g >= 0;
                const unsigned g16 = ((unsigned)p.first + (unsigned)g) & 0xffffu;
                b[i] = ok ? ddc::load_block<RT>(p.src, g, q) : 0;
#pragma unroll
                for (int h = 0; h < 2; ++h) e[i][h] = ok ? p.table[(kr[h] * g16) & (unsigned)(ddc::P - 1)] : 0u;
            }
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const int idx = (rt0 + i) * ddc::ROWS + j;
                if ((rt0 + i) * ddc::ROWS < np) {
                    const long x = b[i] ^ (long)0x8080808080808080UL;
                    const v4i hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.x, a.y), x, zero, 0, 0, 0);
                    const v4i lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.z, a.w), x, zero, 0, 0, 0);
                    if (idx < np) emit_phase(p, ph, hi, lo, c0, e[i], glo - 1 + idx, idx);
                }
            }
        }
    } else {
        uint4* ops = reinterpret_cast<uint4*>(s1_of_ch(lds, 0));
        const int nks = (R + 15) >> 4;
        for (int k = tid; k < nks * 64; k += THREADS) ops[k] = ddc::phasor_operand(p, ct, k >> 6, k & 63);
        __syncthreads();
#pragma unroll 1
        for (int rt = wave; rt < nrt; rt += WAVES) {
            const int idx = rt * ddc::ROWS + j;
            const long g = glo - 1 + idx;
            const bool ok = idx < np && g >= 0;
            const unsigned g16 = ((unsigned)p.first + (unsigned)g) & 0xffffu;
            uint32_t e[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) e[h] = ok ? p.table[(kr[h] * g16) & (unsigned)(ddc::P - 1)] : 0u;
            v4i hi = zero, lo = zero;
#pragma unroll 1
            for (int ks = 0; ks < nks; ++ks) {
                const long x = (ok ? ddc::load_any(p.src, g, R, 16 * ks + 4 * q) : 0) ^ (long)0x8080808080808080UL;
                const uint4 a = ops[ks * 64 + lane];
                hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.x, a.y), x, hi, 0, 0, 0);
                lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.z, a.w), x, lo, 0, 0, 0);
            }
            if (idx < np) emit_phase(p, ph, hi, lo, c0, e, g, idx);
        }
    }
}

// B. the stage-1 streams from s1lo, n1 positions: first difference and limiter, or the carried delay line in front
// of sample 0; even and odd positions in two arrays (fm_chain.hip)
__device__ __forceinline__ void stage1(const BankParams& p, const fm::Maps& m, const fm::TileRange& r, int c_first, int nchl,
                                       float* lds)
{
    const fm::TileMap to_g(r.s1lo < 0 ? 0 : r.s1lo, m.L1, m.L);
    for (int j = threadIdx.x; j < r.n1; j += THREADS) {
        const long s1 = r.s1lo + j;
        const int at = (j & 1 ? S1_HALF : 0) + (j >> 1);
        if (s1 < 0) {
            for (int ch = 0; ch < nchl; ++ch) s1_of_ch(lds, ch)[at] = p.state_in[(c_first + ch) * STATE + 11 + s1];
        } else {
            const int i = (int)(to_g(s1) - r.glo) + 1;
            for (int ch = 0; ch < nchl; ++ch) {
                const float* ph = phase_of_ch(lds, ch);
                s1_of_ch(lds, ch)[at] = fm_limit_dev(ph[i], ph[i - 1]);
            }
        }
    }
}

template <int RT>
__global__ __launch_bounds__(THREADS) void fm_bank_kernel(const BankParams p)
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int tid = threadIdx.x;
    const int nct = (p.nch + COL_CH - 1) / COL_CH;
    const long t = blockIdx.x / (unsigned)nct;
    const int ct = (int)(blockIdx.x - (unsigned)t * (unsigned)nct);
    const int c_first = COL_CH * ct;
    const int nchl = p.nch - c_first < COL_CH ? p.nch - c_first : COL_CH;
    const fm::Maps m = fm::make_maps(p.block_len, p.nblocks);
    const bool tail = t == p.ntiles;
    const fm::TileRange r = tail ? tail_range(m) : fm::tile_range<TILE>(m, t);

    phases<RT>(p, ct, r.glo, r.np, lds);
    __syncthreads();
    stage1(p, m, r, c_first, nchl, lds);
    __syncthreads();

    const fm::TileMap to_w(r.s2lo < 0 ? 0 : r.s2lo, m.L2, m.half);
    if (tail) {
        // state_out of eight channels, 32 threads each: the last ten of the stage-1 stream, the last ten of the
        // stage-2 stream, the phase of the last sample
        const int ch = tid >> 5, i = tid & 31;
        if (ch < nchl) {
            float* out = p.state_out + (long)(c_first + ch) * STATE;
            const float* s1e = s1_of_ch(lds, ch);
            if (i < 10) {
                const int j = (int)(m.nblocks * m.L1 - 10 + i - r.s1lo);
                out[1 + i] = s1e[(j & 1 ? S1_HALF : 0) + (j >> 1)];
            } else if (i < 20) {
                const long s2 = r.s2lo + (i - 10);
                out[1 + i] = work_at(s1e, (int)(to_w(s2) - r.wlo) + 5);
            } else if (i == 20) {
                out[0] = phase_of_ch(lds, ch)[r.np - 1];
            }
        }
        return;
    }

    // C. the stage-2 streams over the phases: the first half-band at the positions the second one reads
    for (int j = tid; j < r.n2; j += THREADS) {
        const long s2 = r.s2lo + j;
        const int at = (j & 1 ? S2_HALF : 0) + (j >> 1);
        if (s2 < 0) {
            for (int ch = 0; ch < nchl; ++ch) phase_of_ch(lds, ch)[at] = p.state_in[(c_first + ch) * STATE + 21 + s2];
        } else {
            const int k = (int)(to_w(s2) - r.wlo) + 5;
            for (int ch = 0; ch < nchl; ++ch) phase_of_ch(lds, ch)[at] = work_at(s1_of_ch(lds, ch), k);
        }
    }
    __syncthreads();

    // D. audio sample a0 + a sits at stage-2 position s2lo + 2 (a + 5)
    for (int a = tid; a < r.na; a += THREADS) {
        const int k = a + 5;
        for (int ch = 0; ch < nchl; ++ch) {
            const float* s2e = phase_of_ch(lds, ch);
            const float* s2o = s2e + S2_HALF;
            p.audio[(long)(c_first + ch) * p.audio_stride + r.a0 + a] =
                halfband_dev(s2o[k - 3], s2e[k], s2e[k - 1], s2e[k - 2], s2e[k - 3], s2e[k - 4], s2e[k - 5]);
        }
    }
}

// the launch table: f is handed the instantiation of cic_r (pick) or every instantiation in turn (visit_all)
template <typename Choice, typename F>
static hipError_t with_kernel(Choice choose, int cic_r, F&& f)
{
    return choose(Vals<0, 8, 10, 12>{}, ddc::rt_of(cic_r), [&](auto rt) { return f(&fm_bank_kernel<rt>); });
}

hipError_t launch_bank(const BankParams& p, hipStream_t st)
{
    const long nct = (p.nch + COL_CH - 1) / COL_CH;
    return with_kernel(pick, p.cic_r,
                       [&](auto kernel) { return launch(kernel, dim3((unsigned)((p.ntiles + 1) * nct)), dim3(THREADS), 0, st, p); });
}

hipError_t launch_state_copy(const float* state_in, float* state_out, int nfloats, hipStream_t st)
{
    hipLaunchKernelGGL(fm_bank_state_copy_kernel, dim3(1), dim3(THREADS), 0, st, state_in, state_out, nfloats);
    return hipGetLastError();
}

// load_kernel (rtlws_internal.h).  The LDS of the kernels is static (above 64 KiB, within the CU's 160 KiB): there is no
// limit to raise.  A plan does not know cic_r: every instantiation, after the state copy
hipError_t prepare_bank()
{
    const hipError_t e = load_kernel(&fm_bank_state_copy_kernel);
    if (e != hipSuccess) return e;
    return with_kernel(visit_all, 0, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace fmbank
}  // namespace rtlws

// fmfir_bank.hip -- up to 32 FM stations from one cmplx_u8 capture behind an int16 FIR as ONE kernel
// (include/rtlws_fmfir.h): the decimated samples of the filtered down-converter bank (ddcfir_bank.hip) are demodulated
// where they are formed, and the chain of fm_chain.hip runs per channel out of LDS.  Nothing between the capture and
// the audio touches device memory.  Built with -ffp-contract=off.
//
// The work split is fm_bank.hip's: a workgroup owns TILE consecutive audio samples of one column tile of eight
// channels, and per column tile one more workgroup, the last, writes state_out.  Only stage A is this file's: the
// decimated samples glo - 1 .. ghi are formed, sixteen at a time per wavefront and PAIR row tiles against one read of
// an operand, with ddcfir_bank.hip's contraction (ddcfir_ops.h: the same operands from T, the words and the taps, the
// same three load forms of a window; ddc_ops.h: the same rotation at 14 + s -- the integers are rtlws_ddcfir_run's).
// ceil(L / 16) K steps go into the high and the low accumulator; the column tile's operands, 1 KiB per K step, lie
// over the stage-1 streams until the barrier behind stage A.  In the accumulator's lane map a lane holds (re, im) of
// two channels of one sample: the conversion to f32 and atan2_approx follow on that lane, and the phase goes to the
// channel's array in LDS (fm_bank_stages.h's emit_phase).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_ops.h"
#include "ddcfir_ops.h"
#include "fm_bank_stages.h"
#include "fmfir.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace fmfir {

using ddc::v4i;
using fmbank::phase_of_ch;
using fmbank::s1_of_ch;
using fmbank::work_at;
using fmbank::PHASE_CAP;
using fmbank::S1_HALF;
using fmbank::S2_HALF;

// A. the phases of decimated samples glo - 1 .. glo - 2 + np of the column tile's channels into LDS.
// ALIGNED: decim and ntaps multiples of four (8-byte operand loads); else any decim 1 .. 128 and ntaps 1 .. 256.
// The block-phasor lookups of a pair of row tiles and the windows of the next K step are in flight ahead of the MFMAs.
template <bool ALIGNED>
__device__ __forceinline__ void phases(const BankParams& p, int ct, long glo, int np, float* lds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int R = p.decim, L = p.ntaps;
    const int nks = ddcfir::k_steps(L);
    const int c0 = COL_CH * ct + 2 * q;
    const int nrt = (np + ddc::ROWS - 1) / ddc::ROWS;
    float* ph = phase_of_ch(lds, 2 * q);
    unsigned kr[2];                                      // k_c R mod P of the channels this lane holds
#pragma unroll
    for (int h = 0; h < 2; ++h) kr[h] = (unsigned)(p.words[(c0 + h) & (MAX_CH - 1)] * R) & 0xffffu;

    uint4* ops = reinterpret_cast<uint4*>(s1_of_ch(lds, 0));
    for (int k = tid; k < nks * 64; k += THREADS) ops[k] = ddcfir::filter_operand(p, ct, k >> 6, k & 63);
    __syncthreads();

#pragma unroll 1
    for (int rt0 = wave * PAIR; rt0 < nrt; rt0 += WAVES * PAIR) {
        long g[PAIR], x[PAIR];
        bool ok[PAIR];
        uint32_t e[PAIR][2];
        v4i hi[PAIR], lo[PAIR];
#pragma unroll
        for (int i = 0; i < PAIR; ++i) {
            const int idx = (rt0 + i) * ddc::ROWS + j;
            g[i] = glo - 1 + idx;
            ok[i] = idx < np && g[i] >= 0;
            const unsigned g16 = ((unsigned)p.first + (unsigned)g[i]) & 0xffffu;
#pragma unroll
            for (int h = 0; h < 2; ++h) e[i][h] = ok[i] ? p.table[(kr[h] * g16) & (unsigned)(ddc::P - 1)] : 0u;
            x[i] = ok[i] ? ddcfir::load_window<ALIGNED>(p.src, g[i], R, L, 4 * q) : 0;
            hi[i] = lo[i] = v4i{0, 0, 0, 0};
        }
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            long next[PAIR];                             // behind the last K step every sample lies beyond L: zero, no load
#pragma unroll
            for (int i = 0; i < PAIR; ++i) next[i] = ok[i] ? ddcfir::load_window<ALIGNED>(p.src, g[i], R, L, 16 * (ks + 1) + 4 * q) : 0;
            const uint4 a = ops[ks * 64 + lane];
#pragma unroll
            for (int i = 0; i < PAIR; ++i) {
                const long b = x[i] ^ (long)0x8080808080808080UL;
                hi[i] = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.x, a.y), b, hi[i], 0, 0, 0);
                lo[i] = __builtin_amdgcn_mfma_i32_16x16x32_i8(ddc::pack(a.z, a.w), b, lo[i], 0, 0, 0);
                x[i] = next[i];
            }
        }
#pragma unroll
        for (int i = 0; i < PAIR; ++i) {
            const int idx = (rt0 + i) * ddc::ROWS + j;
            if (idx < np) fmbank::emit_phase(p, ph, hi[i], lo[i], c0, e[i], g[i], idx);
        }
    }
}

// Stages B - D and the writer of state_out: fm_bank.hip's, in this unit's own spelling (functions that are handed the
// kernel's tile maps; fm_bank_stages.h says why they are not shared)

// B. the stage-1 streams from s1lo, n1 positions: first difference and limiter, or the carried delay line in front
// of sample 0; even and odd positions in two arrays (fm_chain.hip).  to_g: the kernel's map from the stage-1 stream to
// the decimated samples, built from r.s1lo as tests/fm_ref.py's host check builds it
__device__ __forceinline__ void stage1(const BankParams& p, const fm::TileRange& r, const fm::TileMap to_g, int c_first, int nchl,
                                       float* lds)
{
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

// The workgroup behind the last tile, after stage B and its barrier: state_out of eight channels, 32 threads each: the
// last ten of the stage-1 stream, the last ten of the stage-2 stream, the phase of the last sample.  to_w: the kernel's
// map from the stage-2 stream to the first half-band's outputs, built from r.s2lo; c_first: the column tile's first
// channel, nchl: how many it holds.
__device__ __forceinline__ void write_state(const BankParams& p, const fm::Maps& m, const fm::TileRange& r, const fm::TileMap& to_w,
                                            int c_first, int nchl, float* lds)
{
    const int tid = threadIdx.x;
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
}

// C. the stage-2 streams over the phases: the first half-band at the positions the second one reads
__device__ __forceinline__ void stage2(const BankParams& p, const fm::TileRange& r, const fm::TileMap& to_w, int c_first, int nchl,
                                       float* lds)
{
    for (int j = threadIdx.x; j < r.n2; j += THREADS) {
        const long s2 = r.s2lo + j;
        const int at = (j & 1 ? S2_HALF : 0) + (j >> 1);
        if (s2 < 0) {
            for (int ch = 0; ch < nchl; ++ch) phase_of_ch(lds, ch)[at] = p.state_in[(c_first + ch) * STATE + 21 + s2];
        } else {
            const int k = (int)(to_w(s2) - r.wlo) + 5;
            for (int ch = 0; ch < nchl; ++ch) phase_of_ch(lds, ch)[at] = work_at(s1_of_ch(lds, ch), k);
        }
    }
}

// D. audio sample a0 + a sits at stage-2 position s2lo + 2 (a + 5)
__device__ __forceinline__ void write_audio(const BankParams& p, const fm::TileRange& r, int c_first, int nchl, float* lds)
{
    for (int a = threadIdx.x; a < r.na; a += THREADS) {
        const int k = a + 5;
        for (int ch = 0; ch < nchl; ++ch) {
            const float* s2e = phase_of_ch(lds, ch);
            const float* s2o = s2e + S2_HALF;
            p.audio[(long)(c_first + ch) * p.audio_stride + r.a0 + a] =
                halfband_dev(s2o[k - 3], s2e[k], s2e[k - 1], s2e[k - 2], s2e[k - 3], s2e[k - 4], s2e[k - 5]);
        }
    }
}

template <bool ALIGNED>
__global__ __launch_bounds__(THREADS) void fmfir_bank_kernel(const BankParams p)
{
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    const int nct = (p.nch + COL_CH - 1) / COL_CH;
    const long t = blockIdx.x / (unsigned)nct;
    const int ct = (int)(blockIdx.x - (unsigned)t * (unsigned)nct);
    const int c_first = COL_CH * ct;
    const int nchl = p.nch - c_first < COL_CH ? p.nch - c_first : COL_CH;
    const fm::Maps m = fm::make_maps(p.block_len, p.nblocks);
    const bool tail = t == p.ntiles;
    const fm::TileRange r = tail ? fmbank::tail_range(m) : fm::tile_range<TILE>(m, t);

    phases<ALIGNED>(p, ct, r.glo, r.np, lds);
    __syncthreads();
    const fm::TileMap to_g(r.s1lo < 0 ? 0 : r.s1lo, m.L1, m.L);
    stage1(p, r, to_g, c_first, nchl, lds);
    __syncthreads();
    const fm::TileMap to_w(r.s2lo < 0 ? 0 : r.s2lo, m.L2, m.half);
    if (tail) {
        write_state(p, m, r, to_w, c_first, nchl, lds);
        return;
    }
    stage2(p, r, to_w, c_first, nchl, lds);
    __syncthreads();
    write_audio(p, r, c_first, nchl, lds);
}

// the launch table: f is handed the instantiation of (decim, ntaps)
template <typename F>
static hipError_t with_kernel(int decim, int ntaps, F&& f)
{
    return pick(Bools{}, ddcfir::aligned_loads(decim, ntaps), [&](auto aligned) { return f(&fmfir_bank_kernel<aligned>); });
}

hipError_t launch_bank(const BankParams& p, hipStream_t st)
{
    const long nct = (p.nch + COL_CH - 1) / COL_CH;
    return with_kernel(p.decim, p.ntaps,
                       [&](auto kernel) { return launch(kernel, dim3((unsigned)((p.ntiles + 1) * nct)), dim3(THREADS), 0, st, p); });
}

hipError_t launch_state_copy(const float* state_in, float* state_out, int nfloats, hipStream_t st)
{
    hipLaunchKernelGGL(fmbank::fm_bank_state_copy_kernel, dim3(1), dim3(THREADS), 0, st, state_in, state_out, nfloats);
    return hipGetLastError();
}

// load_kernel (rtlws_internal.h).  The LDS of the kernels is static (above 64 KiB, within the CU's 160 KiB): there is no
// limit to raise
hipError_t prepare_bank(int decim, int ntaps)
{
    const hipError_t e = load_kernel(&fmbank::fm_bank_state_copy_kernel);
    if (e != hipSuccess) return e;
    return with_kernel(decim, ntaps, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace fmfir
}  // namespace rtlws

// ddcfir_bank.hip -- a bank of digital down-converters with an int16 FIR as the channel filter, in ONE pass over a
// cmplx_u8 capture (include/rtlws_ddcfir.h): every channel c mixes the capture with exp(-2 pi i k_c n / P), filters
// with the plan's L taps and decimates by R, all in integers.
//
// The arithmetic (P, T as in ddc_bank.hip; h the taps, s the caller's shift):
//   G_c[n]    = ((h[n] T[k_c n mod P] + 2^13 (1 + i)) >> 14                                part by part, |G| <= |h[n]|
//   U[c][m]   = sum_{n<L} (x[m R + n] - 128 (1 + i)) * conj(G_c[n])                        int32, windows overlap
//   out[c][m] = (U[c][m] * conj(T[k_c R g mod P]) + 2^(13+s) (1 + i)) >> (14 + s),  g = first + m
// It is ddc_bank.hip's contraction with K = 2 L bytes per output, D = A B with v_mfma_i32_16x16x32_i8:
//   B (32 x 16)  column j = decimated sample m0 + j, k = byte of K step ks of its window: lane l holds column l & 15,
//                bytes 8 (l >> 4) .. + 7 of the 32 at byte 2 (m R + 16 ks) of the capture, offset binary off by ^ 0x80.
//                Windows of neighbouring columns overlap; they are read from global memory as they are and the L1/L2
//                serve the overlap.  R and L multiples of four: one aligned 8-byte load; else two 4-byte loads where both
//                are even, four 2-byte loads where one is odd;
//   A (16 x 32)  row 2 c' = Re, 2 c' + 1 = Im of channel c' of a column tile of eight channels: (Gc_n, Gs_n) and
//                (-Gs_n, Gc_n) at the bytes of tap n, zero from tap L on.  G = 256 Gh + Gl with Gl in -128 .. 127 and,
//                because |h| <= 32639, Gh in -127 .. 127: two int8 operands, D = 256 (A_h B) + A_l B exactly.  The
//                workgroup builds them from T, the words and the taps at its start and keeps them in LDS, 16 bytes per
//                lane and (column tile, K step): at most 4 x 16 x 1 KiB;
//   D            as in ddc_bank.hip: lane l holds column l & 15 and rows 4 (l >> 4) + i, Re and Im of two channels; the
//                16 lanes of a row group store 128 consecutive bytes of one channel's stream.
// ceil(L / 16) K steps go into the same accumulators; a wavefront takes PAIR row tiles against one read of an operand.
// The builder of A (filter_operand) and the loader of B (load_window) are ddcfir_ops.h's: fmfir_bank.hip compiles them too.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_ops.h"
#include "ddcfir.h"
#include "ddcfir_ops.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace ddcfir {

using ddc::emit;
using ddc::nt_u2;
using ddc::pack;
using ddc::phasor;
using ddc::v4i;

// NCT column tiles of eight channels: the accumulators of PAIR row tiles stay in registers at every NCT
template <bool ALIGNED, int NCT>
__device__ __forceinline__ void bank_tile(const FirParams& p, const uint4* ops, int nks)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int R = p.decim, L = p.ntaps;
    const long tile0 = (long)blockIdx.x * TILE_DEC;

    // k_c R mod P of the channels this lane stores
    unsigned kr[NCT][2];
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
        for (int h = 0; h < 2; ++h) kr[ct][h] = (unsigned)(p.words[(8 * ct + 2 * q + h) & (MAX_CH - 1)] * R) & 0xffffu;

#pragma unroll 1
    for (int it = 0; it < ROW_TILES / (4 * PAIR); ++it) {
        const long m0 = tile0 + (long)((it * 4 + wave) * PAIR) * ROWS;
        if (m0 >= p.dec_len) break;                      // the wavefront's later row tiles lie further on
        long m[PAIR];
        bool valid[PAIR];
        v4i hi[PAIR][NCT], lo[PAIR][NCT];
#pragma unroll
        for (int i = 0; i < PAIR; ++i) {
            m[i] = m0 + i * ROWS + j;
            valid[i] = m[i] < p.dec_len;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) hi[i][ct] = lo[i][ct] = v4i{0, 0, 0, 0};
        }
#pragma unroll 1
        for (int ks = 0; ks < nks; ++ks) {
            long x[PAIR];
#pragma unroll
            for (int i = 0; i < PAIR; ++i)
                x[i] = (valid[i] ? load_window<ALIGNED>(p.src, m[i], R, L, 16 * ks + 4 * q) : 0) ^ (long)0x8080808080808080UL;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct) {
                const uint4 a = ops[(ct * nks + ks) * 64 + lane];
#pragma unroll
                for (int i = 0; i < PAIR; ++i) {
                    hi[i][ct] = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a.x, a.y), x[i], hi[i][ct], 0, 0, 0);
                    lo[i][ct] = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a.z, a.w), x[i], lo[i][ct], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < PAIR; ++i) {
            if (valid[i]) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct) emit(p, hi[i][ct], lo[i][ct], 8 * ct + 2 * q, kr[ct][0], kr[ct][1], m[i]);
            }
        }
    }
}

// ALIGNED: decim and ntaps multiples of four (8-byte operand loads); else any decim 1 .. 128 and ntaps 1 .. 256.
// Dynamic LDS: lds_bytes(ntaps, nch), the operands of the launch's column tiles and K steps
template <bool ALIGNED>
__global__ __launch_bounds__(THREADS) void ddcfir_bank_kernel(const FirParams p)
{
    extern __shared__ __attribute__((aligned(16))) uint4 ops[];
    const int tid = threadIdx.x;
    const int nct = col_tiles(p.nch), nks = k_steps(p.ntaps);
    for (int e = tid; e < nct * nks * 64; e += THREADS) {
        const int ks = (e >> 6) % nks, ct = (e >> 6) / nks;
        ops[e] = filter_operand(p, ct, ks, e & 63);
    }
    __syncthreads();

    if (nct == 1) bank_tile<ALIGNED, 1>(p, ops, nks);
    else if (nct == 2) bank_tile<ALIGNED, 2>(p, ops, nks);
    else if (nct == 3) bank_tile<ALIGNED, 3>(p, ops, nks);
    else bank_tile<ALIGNED, 4>(p, ops, nks);
}

// the launch table: f is handed the instantiation of (decim, ntaps)
template <typename F>
static hipError_t with_kernel(int decim, int ntaps, F&& f)
{
    return pick(Bools{}, aligned_loads(decim, ntaps), [&](auto aligned) { return f(&ddcfir_bank_kernel<aligned>); });
}

hipError_t launch_bank(const FirParams& p, hipStream_t st)
{
    const long blocks = (p.dec_len + TILE_DEC - 1) / TILE_DEC;
    const size_t lds = (size_t)lds_bytes(p.ntaps, p.nch);
    return with_kernel(p.decim, p.ntaps,
                       [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), lds, st, p); });
}

// load_kernel (rtlws_internal.h) for the kernel of a filter.  The largest launch asks for 64 KiB of dynamic LDS, the most
// that lds_opt_in passes without raising a limit
hipError_t prepare_bank(int decim, int ntaps, int device)
{
    return with_kernel(decim, ntaps, [&](auto kernel) {
        const hipError_t e = load_kernel(kernel);
        return e != hipSuccess ? e : lds_opt_in(kernel, device, (size_t)lds_bytes(MAX_TAPS, MAX_CH));
    });
}

}  // namespace ddcfir
}  // namespace rtlws

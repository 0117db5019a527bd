// ddc_bank.hip -- a bank of digital down-converters in ONE pass over a cmplx_u8 capture (include/rtlws_ddc.h):
// every channel c mixes the capture with exp(-2 pi i k_c n / P) and block-sums R samples, all in integers.
// 2 R bytes in and 8 C bytes out per decimated sample, the capture read once whatever C is.
//
// The arithmetic (P = 2^16, T[j] = rint(2^14 (cos, sin)(2 pi j / P)) as int16 pairs):
//   U[c][m]   = sum_{n<R} (x[m R + n] - 128 (1 + i)) * conj(T[k_c n mod P])            int32, inside the block
//   out[c][m] = (U[c][m] * conj(T[k_c R g mod P]) + 2^27 (1 + i)) >> 28,  g = first + m  int64, one per output
// The inner sum is a dense int8 contraction on the matrix pipe.  D = A B with v_mfma_i32_16x16x32_i8:
//   B (32 x 16)  column j = decimated sample m0 + j, k = byte of its block of 2 R bytes (re, im interleaved) with
//                the offset binary taken off by ^ 0x80: lane l holds column l & 15, bytes 8 (l >> 4) .. + 7 --
//                its own eight consecutive bytes of the capture, straight from the load;
//   A (16 x 32)  row 2 c' = Re, 2 c' + 1 = Im of channel c' of a column tile of eight channels: (c_n, s_n) and
//                (-s_n, c_n) at the bytes of sample n.  An int16 phasor is w = 256 wh + wl with wl in -128 .. 127
//                and wh in -64 .. 64: two int8 operands, D = 256 (A_h B) + A_l B exactly;
//   D            lane l holds column l & 15 (the sample) and rows 4 (l >> 4) + i: Re and Im of TWO channels --
//                a complex value stays on its lane, and the 16 lanes of a row group store 128 consecutive bytes
//                of one channel's stream.
// R <= 16 is one K step; the generic kernel takes ceil(R / 16) steps into the same accumulators.  A wavefront
// derives its phasor operands from T itself (R = 8, 10, 12: in registers; any R: the workgroup's, in LDS), so
// a retune is nothing but other kernel arguments.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ddc_bank.h"
#include "ddc_ops.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace ddc {

// RT = 8, 10, 12: that factor, one K step, the phasor operands in registers.  RT = 0: any factor 1 .. 128.
template <int RT>
__global__ __launch_bounds__(THREADS) void ddc_bank_kernel(const BankParams p)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j = lane & 15, q = lane >> 4;
    const int nct = (p.nch + 7) >> 3;
    const int R = RT ? RT : p.cic_r;
    const long tile0 = (long)blockIdx.x * TILE_DEC;

    // k_c R mod P of the channels this lane stores
    unsigned kr[COL_TILES][2];
#pragma unroll
    for (int ct = 0; ct < COL_TILES; ++ct)
#pragma unroll
        for (int h = 0; h < 2; ++h) kr[ct][h] = (unsigned)(p.words[(8 * ct + 2 * q + h) & (MAX_CH - 1)] * R) & 0xffffu;

    if constexpr (RT != 0) {
        uint4 a[COL_TILES];
#pragma unroll
        for (int ct = 0; ct < COL_TILES; ++ct) a[ct] = ct < nct ? phasor_operand(p, ct, 0, lane) : make_uint4(0, 0, 0, 0);

#pragma unroll 1
        for (int gi = 0; gi < ROW_TILES / (4 * GROUP); ++gi) {
            const long m_base = tile0 + (long)((gi * 4 + wave) * GROUP * ROWS);
            if (m_base >= p.dec_len) break;
            long b[GROUP];                               // every load of the group in flight
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const long m = m_base + i * ROWS + j;
                b[i] = m < p.dec_len ? load_block<RT>(p.src, m, q) : 0;
            }
#pragma unroll
            for (int i = 0; i < GROUP; ++i) {
                const long m = m_base + i * ROWS + j;
                if (m_base + i * ROWS < p.dec_len) {
                    const long x = b[i] ^ (long)0x8080808080808080UL;
                    const v4i zero = {0, 0, 0, 0};
#pragma unroll
                    for (int ct = 0; ct < COL_TILES; ++ct) {
                        if (ct < nct) {
                            const v4i hi = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a[ct].x, a[ct].y), x, zero, 0, 0, 0);
                            const v4i lo = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a[ct].z, a[ct].w), x, zero, 0, 0, 0);
                            if (m < p.dec_len) emit(p, hi, lo, 8 * ct + 2 * q, kr[ct][0], kr[ct][1], m);
                        }
                    }
                }
            }
        }
    } else {
        __shared__ uint4 ops[COL_TILES * K_STEPS * 64];
        const int nks = (R + 15) >> 4;
        for (int e = tid; e < nct * nks * 64; e += THREADS) {
            const int ks = (e >> 6) % nks, ct = (e >> 6) / nks;
            ops[(ct * K_STEPS + ks) * 64 + (e & 63)] = phasor_operand(p, ct, ks, e & 63);
        }
        __syncthreads();

#pragma unroll 1
        for (int rt = 0; rt < ROW_TILES / 4; ++rt) {
            const long m0 = tile0 + (long)(((rt / GROUP) * 4 + wave) * GROUP + rt % GROUP) * ROWS;
            if (m0 >= p.dec_len) continue;
            const long m = m0 + j;
            const bool valid = m < p.dec_len;
            v4i hi[COL_TILES], lo[COL_TILES];
#pragma unroll
            for (int ct = 0; ct < COL_TILES; ++ct) hi[ct] = lo[ct] = v4i{0, 0, 0, 0};
#pragma unroll 1
            for (int ks = 0; ks < nks; ++ks) {
                const long x = (valid ? load_any(p.src, m, R, 16 * ks + 4 * q) : 0) ^ (long)0x8080808080808080UL;
#pragma unroll
                for (int ct = 0; ct < COL_TILES; ++ct) {
                    if (ct < nct) {
                        const uint4 a = ops[(ct * K_STEPS + ks) * 64 + lane];
                        hi[ct] = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a.x, a.y), x, hi[ct], 0, 0, 0);
                        lo[ct] = __builtin_amdgcn_mfma_i32_16x16x32_i8(pack(a.z, a.w), x, lo[ct], 0, 0, 0);
                    }
                }
            }
            if (valid) {
#pragma unroll
                for (int ct = 0; ct < COL_TILES; ++ct)
                    if (ct < nct) emit(p, hi[ct], lo[ct], 8 * ct + 2 * q, kr[ct][0], kr[ct][1], m);
            }
        }
    }
}

// the launch table: f is handed the instantiation of cic_r (pick) or every instantiation in turn (visit_all)
template <typename Choice, typename F>
static hipError_t with_kernel(Choice choose, int cic_r, F&& f)
{
    return choose(Vals<0, 8, 10, 12>{}, rt_of(cic_r), [&](auto rt) { return f(&ddc_bank_kernel<rt>); });
}

hipError_t launch_bank(const BankParams& p, hipStream_t st)
{
    const long blocks = (p.dec_len + TILE_DEC - 1) / TILE_DEC;
    return with_kernel(pick, p.cic_r, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

// load_kernel (rtlws_internal.h).  A plan does not know cic_r: every instantiation
hipError_t prepare_bank()
{
    return with_kernel(visit_all, 0, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace ddc
}  // namespace rtlws

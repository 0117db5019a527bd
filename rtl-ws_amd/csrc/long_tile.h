// long_tile.h -- the device text of the four-step transform's tile: ONE text for the kernels of spectrum_long.hip
// (librtlws_long.so) and spectrum_anylen.hip (librtlws_anylen.so), as fm_math.h is for the FM chain.  The tile
// layout, the thread maps and the global access patterns are described in spectrum_long.hip's header comment.
#ifndef RTLWS_LONG_TILE_H
#define RTLWS_LONG_TILE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs_f64.h"
#include "spectrum_long.h"

namespace rtlws {
namespace lng {

typedef double2 d2;

template <int T>
__device__ __forceinline__ int swz(int pos)
{
    if constexpr (T == 8) return pos ^ ((pos >> 2) & 1);
    else return pos;
}

// 8-point forward DFT over v[B .. B+7]: input slot n holds x[n], output slot s holds X[rev8(s)]
template <int B>
__device__ __forceinline__ void fft8(d2 (&v)[16])
{
    f64::bfly4(v[B + 0], v[B + 2], v[B + 4], v[B + 6]);
    f64::bfly4(v[B + 1], v[B + 3], v[B + 5], v[B + 7]);
    v[B + 3] = f64::mul_w16<2>(v[B + 3]);
    v[B + 5] = f64::mul_w16<4>(v[B + 5]);
    v[B + 7] = f64::mul_w16<6>(v[B + 7]);
#pragma unroll
    for (int p = 0; p < 4; ++p) f64::bfly2(v[B + 2 * p], v[B + 2 * p + 1]);
}

// the frequency index of register `slot` of thread group gi after tile_fft
template <int LOG2L>
__device__ __forceinline__ int out_k(int gi, int slot)
{
    if constexpr (LOG2L == 7) {
        return gi + 8 * (slot >> 3) + 16 * f64::rev8(slot & 7);
    } else if constexpr (LOG2L == 8) {
        return gi + 16 * f64::rev16(slot);
    } else {
        constexpr int R = 1 << (LOG2L - 8), G = 1 << (LOG2L - 4);
        const int c = gi + G * (slot / R);
        return (c >> 4) + 16 * (c & 15) + 256 * (slot % R);
    }
}

// The T L-point transforms of the tile in LDS (natural order, element (pos, col) at swz(pos) * T + col).  On return
// register v[slot] of thread t holds X[out_k(t / T, slot)] of column t % T; the LDS holds intermediate values.
template <int LOG2L>
__device__ __forceinline__ void tile_fft(d2* xs, const d2* __restrict__ twc, int t, d2 (&v)[16])
{
    constexpr int L = 1 << LOG2L, T = TILE_POINTS / L, G = L / 16;
    const int col = t % T, gi = t / T;
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = xs[swz<T>(gi + q * G) * T + col];
    f64::fft16_sel(v);
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int p = f64::rev16(s);
        d2 y = v[s];
        if (p) y = f64::cmul(y, twc[(gi * p) << (10 - LOG2L)]);          // W_L^(gi p)
        xs[swz<T>(gi + p * G) * T + col] = y;
    }
    __syncthreads();
    if constexpr (LOG2L >= 9) {
        constexpr int M2 = L / 16, J = M2 / 16;                          // sixteen blocks of M2 = 32 | 64 points
        const int j = gi % J, base = (gi / J) * M2 + j;
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = xs[swz<T>(base + q * J) * T + col];
        f64::fft16_sel(v);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int p = f64::rev16(s);
            d2 y = v[s];
            if (p) y = f64::cmul(y, twc[(j * p) * (1024 / M2)]);         // W_M2^(j p)
            xs[swz<T>(base + p * J) * T + col] = y;
        }
        __syncthreads();
        constexpr int R = J, U = 16 / R;                                 // 256 blocks of R = 2 | 4 points
#pragma unroll
        for (int u = 0; u < U; ++u)
#pragma unroll
            for (int q = 0; q < R; ++q) v[R * u + q] = xs[swz<T>(R * (gi + u * G) + q) * T + col];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if constexpr (R == 2) f64::bfly2(v[2 * u], v[2 * u + 1]);
            else f64::bfly4(v[4 * u], v[4 * u + 1], v[4 * u + 2], v[4 * u + 3]);
        }
    } else if constexpr (LOG2L == 8) {
#pragma unroll
        for (int q = 0; q < 16; ++q) v[q] = xs[(16 * gi + q) * T + col];
        f64::fft16_sel(v);
    } else {
#pragma unroll
        for (int u = 0; u < 2; ++u)
#pragma unroll
            for (int q = 0; q < 8; ++q) v[8 * u + q] = xs[(8 * (gi + 8 * u) + q) * T + col];
        fft8<0>(v);
        fft8<8>(v);
    }
}

// sample i of the group's input as the reference converts it
template <int IN>
__device__ __forceinline__ d2 load_sample(const void* in, long i, double scale)
{
    if constexpr (IN == IN_CS32) {
        const int2 s = reinterpret_cast<const int2*>(in)[i];
        return make_double2((double)s.x * scale, (double)s.y * scale);
    } else if constexpr (IN == IN_RF32) {
        return make_double2((double)reinterpret_cast<const float*>(in)[i] * scale, 0.0);
    } else {
        const uchar2 s = reinterpret_cast<const uchar2*>(in)[i];
        return make_double2((double)((int)s.x - 128) * scale, (double)((int)s.y - 128) * scale);   // /128: exact
    }
}

// Workgroups go to the eight XCDs (one L2 each) in turn.  Where pass A's runs are shorter than a 128-byte line, the
// neighbouring tiles read the rest of it: with the grid dealt in eight contiguous chunks, one per XCD, they do so
// through the same L2 at about the same time, instead of every tile fetching the whole line through its own
// (measured before: 8 x the input bytes at N1 = 1024, profiles/long_frames_rates.txt).  Bijective when the grid
// is a multiple of 8 -- every m >= 16 -- and the identity otherwise.
__device__ __forceinline__ unsigned xcd_chunked(unsigned bid, unsigned n)
{
    return (n % 8u) ? bid : (bid % 8u) * (n / 8u) + bid / 8u;
}

// one row value through the epilogue the descriptor asks for (P: LongParams, or another struct with its out,
// out_mode, k_avg and lin_gain fields)
template <int ROWS, typename P>
__device__ __forceinline__ void store_value(const P& p, long i, double a)
{
    if constexpr (ROWS == ROWS_U8) {
        const uint8_t o[1] = {(uint8_t)payload_f64(p.lin_gain * a, p.k_avg)};
        store_nt(reinterpret_cast<uint8_t*>(p.out) + i, o);
    } else {
        const double o = (p.out_mode == OUT_DB) ? db_f64(a, p.k_avg) : a;
        if constexpr (ROWS == ROWS_F32) {
            const float o32[1] = {(float)o};                             // RTLWS_FLAG_ROWS_F32: one rounding, on the store
            store_nt(reinterpret_cast<float*>(p.out) + i, o32);
        } else {
            const double o64[1] = {o};
            store_nt(reinterpret_cast<double*>(p.out) + i, o64);
        }
    }
}

}  // namespace lng
}  // namespace rtlws
#endif

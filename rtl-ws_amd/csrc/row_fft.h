// row_fft.h -- an M-point complex forward FFT of one row held in LDS, M = 2^9 .. 2^14, by a whole workgroup, built from
// fft_regs.h's register butterflies.  The row form of the polyphase family's tile passes (pfb_tile.h),
// written beside them: a row of up to 16 384 points instead of a tile of short rows, decimation in frequency, in place,
// two or three radix-16 passes and a last pass of radix 1, 2, 4 or 8:
//   M = 2^9 .. 2^11:  16 * 16 * R,      R = 2, 4, 8         M = 2^12 .. 2^14:  16 * 16 * 16 * R,  R = 1, 2, 4
// A pass of radix r over blocks of L points takes x[j + n L / r], n < r, to W_L^(j q) sum_n x[..] W_r^(n q) at
// j + q L / r: block q of L / r points then holds the bins q + r k'.  After the last pass the place
//   pos(k) = q1 M / 16 + q2 M / 256 (+ q3 M / 4096) + q_last,   k = q1 + 16 q2 (+ 256 q3) + 16^passes q_last
// holds bin k.  Point i of the row lies at place(i) = i + (i >> 4), as in the family's tiles.  The twiddles come from one
// table e^(-2 pi i j / (2 M)), j < M (the caller's: the real-input untangling reads the same table).
#ifndef RTLWS_ROW_FFT_H
#define RTLWS_ROW_FFT_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs.h"

namespace rtlws {
namespace rowfft {

__device__ __forceinline__ int place(int i) { return i + (i >> 4); }

template <int LOG2M> struct Shape {
    static_assert(LOG2M >= 9 && LOG2M <= 14, "M = 2^9 .. 2^14");
    static constexpr int M = 1 << LOG2M;
    static constexpr bool THREE = LOG2M >= 12;               // three radix-16 passes
    static constexpr int R = 1 << (THREE ? LOG2M - 12 : LOG2M - 8);
    static constexpr int TILE_F2 = M + M / 16;               // float2 places of the row
};

// e^(-2 pi i e / (2 M)) for e < 2 M from the half table
template <int M>
__device__ __forceinline__ f2 root(const float2* tw, int e)
{
    const float2 w = tw[e & (M - 1)];
    return e < M ? mk(w.x, w.y) : mk(-w.x, -w.y);
}

// 8-point forward DFT in registers: slot s < 4 holds X[2 s], slot 4 + s holds X[2 s + 1]
__device__ __forceinline__ void fft8(f2 (&v)[8])
{
#pragma unroll
    for (int i = 0; i < 4; ++i) bfly2(v[i], v[4 + i]);
    v[5] = mul_w16<2>(v[5]);
    v[6] = mul_w16<4>(v[6]);
    v[7] = mul_w16<6>(v[7]);
    bfly4(v[0], v[1], v[2], v[3]);
    bfly4(v[4], v[5], v[6], v[7]);
}

// Butterfly b of the radix-16 pass over blocks of L points (b < M / 16), in place: the thread owns the places it reads
template <int M, int L>
__device__ __forceinline__ void pass16(float2* row, int b, const float2* tw)
{
    constexpr int STRIDE = L / 16;
    const int j = b & (STRIDE - 1), i0 = (b / STRIDE) * L + j;
    f2 v[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) v[n] = row[place(i0 + n * STRIDE)];
    fft16_fma(v);
    if constexpr (L > 16) {
        // W_L^(j q) = e^(-2 pi i j q (2 M / L) / (2 M))
#pragma unroll
        for (int s = 1; s < 16; ++s) v[s] = cmul(v[s], root<M>(tw, j * rev16(s) * (2 * M / L)));
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) row[place(i0 + rev16(s) * STRIDE)] = v[s];
}

// The last pass over the 16 consecutive points from 16 b on: 16 / R transforms of R points, no twiddle behind them
template <int R>
__device__ __forceinline__ void pass_last(float2* row, int b)
{
    if constexpr (R > 1) {
        float2* at = row + place(16 * b);                    // one group of 16: consecutive places
        f2 v[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = at[n];
        if constexpr (R == 2) {
#pragma unroll
            for (int g = 0; g < 8; ++g) bfly2(v[2 * g], v[2 * g + 1]);
        } else if constexpr (R == 4) {
#pragma unroll
            for (int g = 0; g < 4; ++g) bfly4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
        } else {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                f2 y[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) y[r] = v[8 * g + r];
                fft8(y);
#pragma unroll
                for (int s = 0; s < 4; ++s) v[8 * g + 2 * s] = y[s], v[8 * g + 2 * s + 1] = y[4 + s];
            }
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) at[n] = v[n];
    }
}

// The whole transform.  Every thread of the workgroup calls it (tid = threadIdx.x, at least M / 16 threads); the row's
// writers are behind a barrier of the caller's, and every thread has passed the closing barrier on return.
template <int LOG2M>
__device__ __forceinline__ void forward(float2* row, int tid, const float2* tw)
{
    using S = Shape<LOG2M>;
    constexpr int M = S::M;
    const bool mine = tid < M / 16;
    if (mine) pass16<M, M>(row, tid, tw);
    __syncthreads();
    if (mine) pass16<M, M / 16>(row, tid, tw);
    __syncthreads();
    if constexpr (S::THREE) {
        if (mine) pass16<M, M / 256>(row, tid, tw);
        __syncthreads();
    }
    if constexpr (S::R > 1) {
        if (mine) pass_last<S::R>(row, tid);
        __syncthreads();
    }
}

// where bin k lies afterwards (a point index: the place is place(pos(k)))
template <int LOG2M>
__device__ __forceinline__ int pos(int k)
{
    using S = Shape<LOG2M>;
    constexpr int M = S::M;
    if constexpr (S::THREE) return (k & 15) * (M / 16) + ((k >> 4) & 15) * (M / 256) + ((k >> 8) & 15) * (M / 4096) + (k >> 12);
    else return (k & 15) * (M / 16) + ((k >> 4) & 15) * (M / 256) + (k >> 8);
}

// ---- the inverse: from forward's order back to natural order ----
// forward is a product of passes A = A_last .. A_2 A_1 that leaves bin k at pos(k); what takes that order back to the
// points, sum_k Z[k] e^(+2 pi i n k / M) at point n (not scaled by 1 / M), is its conjugate transpose
// A^H = A_1^H A_2^H .. A_last^H: the passes in reverse order, each one decimation in time -- a thread reads the places it
// wrote in forward, value q at j + q L / r, multiplies by the conjugate twiddle W_L^(-j q), takes the conjugate r-point
// transform over q and writes point n at j + n L / r, the places it read in forward.  No reordering pass.  The conjugate
// transform is the forward one between two exchanges of the real and the imaginary part, swap(z) = i conj(z), which
// cost nothing and round nothing; and swap(conj(w) z) = w swap(z), so the table's own entry multiplies the exchanged
// value: the same butterflies, the same table, the same count of roundings as forward.
__device__ __forceinline__ f2 swap(f2 z) { return mk(z.y, z.x); }

template <int M, int L>
__device__ __forceinline__ void inverse_pass16(float2* row, int b, const float2* tw)
{
    constexpr int STRIDE = L / 16;
    const int j = b & (STRIDE - 1), i0 = (b / STRIDE) * L + j;
    f2 v[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) v[q] = swap(row[place(i0 + q * STRIDE)]);
    if constexpr (L > 16) {
#pragma unroll
        for (int q = 1; q < 16; ++q) v[q] = cmul(v[q], root<M>(tw, j * q * (2 * M / L)));
    }
    fft16_fma(v);
#pragma unroll
    for (int s = 0; s < 16; ++s) row[place(i0 + rev16(s) * STRIDE)] = swap(v[s]);
}

// the conjugate of pass_last: the same R-point transforms (natural order in and out) between the two exchanges
template <int R>
__device__ __forceinline__ void inverse_pass_last(float2* row, int b)
{
    if constexpr (R > 1) {
        float2* at = row + place(16 * b);
        f2 v[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = swap(at[n]);
        if constexpr (R == 2) {
#pragma unroll
            for (int g = 0; g < 8; ++g) bfly2(v[2 * g], v[2 * g + 1]);
        } else if constexpr (R == 4) {
#pragma unroll
            for (int g = 0; g < 4; ++g) bfly4(v[4 * g], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
        } else {
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                f2 y[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) y[r] = v[8 * g + r];
                fft8(y);
#pragma unroll
                for (int s = 0; s < 4; ++s) v[8 * g + 2 * s] = y[s], v[8 * g + 2 * s + 1] = y[4 + s];
            }
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) at[n] = swap(v[n]);
    }
}

// The whole inverse, called as forward is: place(pos(k)) holds Z[k] on entry (its writers behind a barrier of the
// caller's), place(n) holds sum_k Z[k] e^(+2 pi i n k / M) on return, and every thread has passed the closing barrier.
template <int LOG2M>
__device__ __forceinline__ void inverse(float2* row, int tid, const float2* tw)
{
    using S = Shape<LOG2M>;
    constexpr int M = S::M;
    const bool mine = tid < M / 16;
    if constexpr (S::R > 1) {
        if (mine) inverse_pass_last<S::R>(row, tid);
        __syncthreads();
    }
    if constexpr (S::THREE) {
        if (mine) inverse_pass16<M, M / 256>(row, tid, tw);
        __syncthreads();
    }
    if (mine) inverse_pass16<M, M / 16>(row, tid, tw);
    __syncthreads();
    if (mine) inverse_pass16<M, M>(row, tid, tw);
    __syncthreads();
}

}  // namespace rowfft
}  // namespace rtlws
#endif

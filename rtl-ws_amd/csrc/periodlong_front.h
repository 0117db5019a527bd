// periodlong_front.h -- the two stages of the long-frame search that read the caller's series (the mean's partial sums
// and the columns), as __device__ templates over where a sample comes from.  periodlong.hip instantiates
// them over the series as it lies (Plain); accel.hip over a series read through a quadratic index map.
// The additions of the mean and the arithmetic of point() are this one text in both, so that a search through the map
// has the bits of the search of the materialised series.
//
// A source has  float one(int n)  sample n,  float2 pair(int n)  samples n (even) and n + 1,  float4 quad(int n)  samples
// n (a multiple of 4) .. n + 3; the callers never ask for a sample at or behind nsamp.
#ifndef RTLWS_CSRC_PERIODLONG_FRONT_H
#define RTLWS_CSRC_PERIODLONG_FRONT_H

#include <hip/hip_runtime.h>

#include "periodlong.h"
#include "row_fft.h"

namespace rtlws {
namespace periodlong {
namespace front {

// the series where it lies: the vector loads of an aligned row
struct Plain {
    const float* x;
    __device__ __forceinline__ float one(int n) const { return x[n]; }
    __device__ __forceinline__ float2 pair(int n) const { return *reinterpret_cast<const float2*>(x + n); }
    __device__ __forceinline__ float4 quad(int n) const { return *reinterpret_cast<const float4*>(x + n); }
};

// the trial's mean from its 64 partial sums: the same additions in every lane, wavefront and workgroup
__device__ __forceinline__ double mean_of(const double* sums, int nsamp)
{
    static_assert(MEAN_PARTS == LANES, "a lane a partial sum");
    double s = sums[threadIdx.x & (LANES - 1)];
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) s += __shfl_xor(s, off);
    return s / (double)nsamp;
}

// the packed point j of a trial: y[2 j] + i y[2 j + 1], nothing at or behind nsamp read, zeros there
template <typename Src>
__device__ __forceinline__ f2 point(const Src& x, long j, int nsamp, double mean)
{
    const long n0 = 2 * j;
    float a = 0.0f, b = 0.0f;
    if (n0 + 2 <= nsamp) {
        const float2 v = x.pair((int)n0);
        a = (float)((double)v.x - mean), b = (float)((double)v.y - mean);
    } else if (n0 < nsamp) {
        a = (float)((double)x.one((int)n0) - mean);
    }
    return mk(a, b);
}

// ---- mean: workgroup (q, slot) sums samples q N / 64 .. (q + 1) N / 64 - 1 below nsamp ----
template <typename Src>
__device__ __forceinline__ void mean(const Params& p, const Src& x)
{
    __shared__ double wsum[MEAN_THREADS / LANES];
    const int tid = threadIdx.x, lane = tid & (LANES - 1), wave = tid / LANES;
    const int nsamp = p.nsamp, per = 1 << (p.log2n - 6), first = (int)blockIdx.x * per;
    double sum = 0.0;
    for (int n0 = first + 4 * tid; n0 < first + per; n0 += 4 * MEAN_THREADS) {
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n0 + 4 <= nsamp) {
            v = x.quad(n0);
        } else if (n0 < nsamp) {                             // the last, partial quad: nothing at or behind nsamp is read
            v.x = x.one(n0);
            if (n0 + 1 < nsamp) v.y = x.one(n0 + 1);
            if (n0 + 2 < nsamp) v.z = x.one(n0 + 2);
        }
        sum += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) sum += __shfl_xor(sum, off);
    if (lane == 0) wsum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        double total = 0.0;
#pragma unroll
        for (int w = 0; w < MEAN_THREADS / LANES; ++w) total += wsum[w];
        p.sums[(long)blockIdx.y * MEAN_PARTS + blockIdx.x] = total;
    }
}

// ---- cols, M1 = 16: a thread a column ----
template <typename Src>
__device__ __forceinline__ void cols16(const Params& p, const Src& x)
{
    const int log2m2 = p.log2n - 5, m2 = 1 << log2m2;
    const long m = 16L << log2m2;
    const int j2 = (int)blockIdx.x * COLS_THREADS + (int)threadIdx.x;
    const double mean = mean_of(p.sums + (long)blockIdx.y * MEAN_PARTS, p.nsamp);
    f2 v[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) v[n] = point(x, (long)n * m2 + j2, p.nsamp, mean);
    fft16_fma(v);
    float2* const z = p.z + (long)blockIdx.y * m + j2;
#pragma unroll
    for (int s = 0; s < 16; ++s) {
        const int k1 = rev16(s);
        if (s) {
            const float2 w = p.twist[(long)k1 * m2 + j2];
            v[s] = cmul(v[s], mk(w.x, w.y));
        }
        z[(long)k1 * m2] = make_float2(v[s].x, v[s].y);
    }
}

// ---- cols, M1 = 256: a workgroup 16 columns; j1 = a + 16 n, k1 = q + 16 q2 ----
template <typename Src>
__device__ __forceinline__ void cols256(const Params& p, const Src& x)
{
    extern __shared__ float4 lds[];
    float2* const tile = reinterpret_cast<float2*>(lds);     // [256][17]
    constexpr int PITCH = COLS256_TILE + 1;
    const int log2m2 = p.log2n - 9, m2 = 1 << log2m2;
    const long m = 256L << log2m2;
    const int tid = threadIdx.x, c = tid & 15, hi = tid >> 4;
    const int j2 = (int)blockIdx.x * COLS256_TILE + c;
    const double mean = mean_of(p.sums + (long)blockIdx.y * MEAN_PARTS, p.nsamp);
    f2 v[16];
    {
        const int a = hi;
#pragma unroll
        for (int n = 0; n < 16; ++n) v[n] = point(x, (long)(a + 16 * n) * m2 + j2, p.nsamp, mean);
        fft16_fma(v);
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int q = rev16(s);
            if (s) {
                const float2 w = p.tw256[a * q];             // a q <= 225
                v[s] = cmul(v[s], mk(w.x, w.y));
            }
            tile[(q * 16 + a) * PITCH + c] = make_float2(v[s].x, v[s].y);
        }
    }
    __syncthreads();
    {
        const int q = hi;
#pragma unroll
        for (int a = 0; a < 16; ++a) v[a] = tile[(q * 16 + a) * PITCH + c];
        fft16_fma(v);
        float2* const z = p.z + (long)blockIdx.y * m + j2;
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            const int k1 = q + 16 * rev16(s);
            const float2 w = p.twist[(long)k1 * m2 + j2];    // row 0 holds ones
            v[s] = cmul(v[s], mk(w.x, w.y));
            z[(long)k1 * m2] = make_float2(v[s].x, v[s].y);
        }
    }
}

}  // namespace front
}  // namespace periodlong
}  // namespace rtlws
#endif

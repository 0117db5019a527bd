// pfb_tile.h -- passes 1-4 of the polyphase filter bank's tile: the integer branch filters, the
// radix-16 passes and the radix-R pass with its reordering.  The one text of pfb_bank.hip (librtlws_pfb.so: pass 5
// stores the tile), pfbspec.hip, pfbxc.hip and pfbbf.hip (their epilogues square, multiply and sum it through
// pfb_ksum.h); and the head of every launch table of the family.
#ifndef RTLWS_PFB_TILE_H
#define RTLWS_PFB_TILE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fft_regs.h"
#include "pfb_bank.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace pfb {

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

// place of point i in a row of the tile (pfb_bank.h)
__device__ __forceinline__ int place(int i) { return i + (i >> 4); }

// radix 16 over the points i0 + n * stride of a row, in place; output k1 is multiplied by tw[k1 * tw_step]
// (tw_step == 0: none)
__device__ __forceinline__ void pass16(float2* row, int i0, int stride, const float2* tw, int tw_step)
{
    f2 v[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) v[n] = row[place(i0 + n * stride)];
    fft16_fma(v);
    if (tw_step != 0) {
#pragma unroll
        for (int s = 1; s < 16; ++s) v[s] = cmul(v[s], tw[rev16(s) * tw_step]);
    }
#pragma unroll
    for (int s = 0; s < 16; ++s) row[place(i0 + rev16(s) * stride)] = v[s];
}

// Branches pc .. pc + 3 of the four consecutive frames mf .. mf + 3 (S = M / hop = 1 or 2).  Frame j and tap t take
// the four samples at row u = j + S t of the thread's column, a row being hop samples: the rows slide through a
// window of four rows in registers (row u in slot u & 3, eight bytes as loaded), so a row is loaded once and used
// by up to four frames.  The bytes are multiplied as they are, 0 .. 255; the offset binary comes off at the end as
// 128 sum_t h[p + t M] (the sums stay below 2^31: 32 * 32768 * 255).  A row that reaches behind the capture is
// needed by no frame of the run and is not loaded.
template <int S, int M>
__device__ __forceinline__ void branch_filters(const PfbParams& p, long mf, int pc, int (&acc)[4][8])
{
    constexpr int D = M / S;
    const unsigned char* src = static_cast<const unsigned char*>(p.src);
    const int T = p.taps_per_branch;
    const long nsamples = (p.nframes - 1) * D + (long)T * M;
    const long base = mf * D + pc;
    auto load_row = [&](int u) {
        const long s0 = base + (long)u * D;
        return s0 + 4 <= nsamples ? *reinterpret_cast<const uint2*>(src + 2 * s0) : make_uint2(0, 0);
    };
    uint2 x[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) x[u] = load_row(u);
    int hsum[4] = {0, 0, 0, 0};
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = 0;
    for (int t0 = 0; t0 < T; t0 += 4) {
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            const int t = t0 + tt;
            if (t < T) {
                const uint2 hw = *reinterpret_cast<const uint2*>(p.taps + t * M + pc);
                const int h[4] = {(int16_t)(hw.x & 0xffffu), (int16_t)(hw.x >> 16), (int16_t)(hw.y & 0xffffu), (int16_t)(hw.y >> 16)};
#pragma unroll
                for (int i = 0; i < 4; ++i) hsum[i] += h[i];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const uint2 xw = x[(j + S * tt) & 3];
                    const unsigned w[2] = {xw.x, xw.y};
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[j][i] += h[i >> 1] * (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu);
                }
                if (t + 1 < T) {
#pragma unroll
                    for (int r = 0; r < S; ++r) x[(S * tt + r) & 3] = load_row(S * t + 4 + r);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] -= 128 * hsum[i >> 1];
}

// Passes 1-4 over the tile of the tile_frames(K) frames from m0 on: afterwards place(c) of row f holds
// Y[m0 + f][c] before the sign rule, and every thread has passed the closing barrier.  The whole workgroup calls it, tid = threadIdx.x;
// the caller keeps the tile's previous readers behind a barrier of its own.  Frames at or behind p.nframes read no
// byte behind the capture (their rows hold values no caller uses).
template <int K>
__device__ __forceinline__ void tile_passes(const PfbParams& p, long m0, int tid, float2* tile)
{
    constexpr int M = 1 << K, ROW = row_stride(K), N2 = M / 16;
    constexpr bool TWO = K >= 8;                      // two radix-16 passes
    constexpr int R = 1 << (TWO ? K - 8 : K - 4);     // what is left for the last pass: 1, 2, 4, 8

    // 1: the branch filters
    {
        constexpr int CG = M / 4;                                 // column groups; THREADS / CG = F / 4 frame groups
        const int pc = (tid % CG) * 4, f0 = (tid / CG) * 4;
        int acc[4][8];
        if (p.half_hop) branch_filters<2, M>(p, m0 + f0, pc, acc);
        else branch_filters<1, M>(p, m0 + f0, pc, acc);
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i)
                tile[(f0 + j) * ROW + place(pc + i)] = make_float2((float)acc[j][2 * i], (float)acc[j][2 * i + 1]);
    }
    __syncthreads();

    // 2: radix 16 at stride N2 of row f; thread (f, n2) owns the places it reads
    {
        const int f = tid / N2, n2 = tid % N2;
        pass16(tile + f * ROW, n2, N2, p.tw, N2 > 1 ? n2 : 0);
    }

    // 3: radix 16 inside block k1 of N2 points at stride N3
    if constexpr (TWO) {
        constexpr int N3 = N2 / 16;
        __syncthreads();
        const int f = tid / N2, j = tid % N2, k1 = j / N3, n3 = j % N3;
        pass16(tile + f * ROW, k1 * N2 + n3, N3, p.tw, N3 > 1 ? 16 * n3 : 0);
    }

    // 4: radix R over the 16 / R blocks tid, tid + 256, ..; then place q * R + kl of a row holds bin
    //    q + 16 kl (one radix-16 pass: q = k1) or (q >> 4) + 16 (q & 15) + 256 kl (two: q = 16 k1 + k2)
    if constexpr (K != 4) {
        constexpr int NB = 16 / R, BPR = M / R;                   // blocks per thread, blocks per row
        f2 w[16];
        __syncthreads();
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            const int blk = tid + THREADS * jb;
            const float2* src = tile + (blk / BPR) * ROW;
#pragma unroll
            for (int r = 0; r < R; ++r) w[jb * R + r] = src[place((blk % BPR) * R + r)];
        }
        if constexpr (R == 2) {
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) bfly2(w[2 * jb], w[2 * jb + 1]);
        } else if constexpr (R == 4) {
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) bfly4(w[4 * jb], w[4 * jb + 1], w[4 * jb + 2], w[4 * jb + 3]);
        } else if constexpr (R == 8) {
#pragma unroll
            for (int jb = 0; jb < NB; ++jb) {
                f2 y[8];
#pragma unroll
                for (int r = 0; r < 8; ++r) y[r] = w[8 * jb + r];
                fft8(y);
#pragma unroll
                for (int r = 0; r < 8; ++r) w[8 * jb + r] = y[r];
            }
        }
        __syncthreads();
#pragma unroll
        for (int jb = 0; jb < NB; ++jb) {
            const int blk = tid + THREADS * jb, q = blk % BPR;
            float2* row = tile + (blk / BPR) * ROW;
            const int c0 = TWO ? (q >> 4) + 16 * (q & 15) : q;
#pragma unroll
            for (int s = 0; s < R; ++s) {
                const int kl = R == 8 ? 2 * (s & 3) + (s >> 2) : s;
                row[place(c0 + (TWO ? 256 : 16) * kl)] = w[jb * R + s];
            }
        }
    }
    __syncthreads();
}

// The launch tables' first choice (rtlws_internal.h): log2 M, a template parameter of every kernel of the family
using Log2Ms = Vals<4, 5, 6, 7, 8, 9, 10>;
static_assert(MIN_LOG2_M == 4 && MAX_LOG2_M == 10, "pfb_bank.h and the launch tables disagree");

// A plan's prepare step is load_kernel (rtlws_internal.h) alone.  The tiles are static LDS, which a launch takes up to the
// 160 KiB of a compute unit as it is: the opt-in of lds_opt_in is for dynamic LDS and has nothing to raise here

}  // namespace pfb
}  // namespace rtlws
#endif

// fm_chain.hip -- the FM receive chain of reference src/audio_main.c:110-142 as ONE kernel (include/rtlws_fm.h):
// [CIC block sums ->] atan2_approx -> first difference, hard limit -> half-band -> half-band, over any number of
// consecutive decimator blocks.  2 * cic_r bytes (or 8) in and one byte out per decimated sample; nothing in between
// touches device memory.  Built with -ffp-contract=off: every float equals the reference's per-block evaluation.
//
// The per-block semantics are one continuous filter over concatenated, truncated streams (L = block_len,
// half = L / 2, quarter = half / 2; tests/test_fm_cpu.py restates the maps in numpy against the oracle):
//   demod[g]   = limit(phase[g] - phase[g-1]),                            phase[-1] = state[0]
//   stage1[s1] = demod[b L + j],      s1 = b (2 half) + j, j < 2 half     (an odd last sample of a block is skipped)
//   work[w]    = halfband(stage1)[w],                                     stage1[-10..-1] = state[1..10]
//   stage2[s2] = work[b half + j],    s2 = b (2 quarter) + j              (an odd last output of a block is skipped)
//   audio[a]   = halfband(stage2)[a],                                     stage2[-10..-1] = state[11..20]
// A workgroup owns TILE consecutive audio samples: it walks the maps back to the range of samples it needs, computes
// each phase once into LDS, and runs the three stages out of LDS.  A stream is kept as two arrays, its even and its
// odd positions: a half-band reads x[2n - k], which from one array would be a stride of two dwords -- a two-way
// bank conflict on every ds_read_b32 (32 banks per 32-lane group); from the split arrays every read is stride one.
// One more workgroup, the last of the grid, evaluates the tails of the three streams straight from device memory
// and writes state_out; state_in and state_out differ, so there is no ordering between workgroups.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "fm_chain.h"
#include "fm_maps.h"
#include "fm_math.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace fm {

typedef unsigned nt_u4 __attribute__((ext_vector_type(4)));
typedef unsigned nt_u2 __attribute__((ext_vector_type(2)));
typedef int nt_i2 __attribute__((ext_vector_type(2)));

// Decimated sample g.  cmplx_u8 sources: the sum over R consecutive samples of (x - 128) per component
// (reference src/resample.c:21-40 without its delay lines), an integer sum in any order.  Streamed once: nontemporal.
template <int SRC>
__device__ __forceinline__ int2 load_sample(const void* src, long g, int R)
{
    if constexpr (SRC == SRC_CS32) {
        const nt_i2 v = __builtin_nontemporal_load(reinterpret_cast<const nt_i2*>(src) + g);
        return make_int2(v.x, v.y);
    } else if constexpr (SRC == SRC_CU8_8) {             // one 16-byte load
        const nt_u4 s = __builtin_nontemporal_load(reinterpret_cast<const nt_u4*>(src) + g);
        unsigned si = 0, sq = 0;
        si = __builtin_amdgcn_udot4(s.x, 0x00010001u, si, false);
        sq = __builtin_amdgcn_udot4(s.x, 0x01000100u, sq, false);
        si = __builtin_amdgcn_udot4(s.y, 0x00010001u, si, false);
        sq = __builtin_amdgcn_udot4(s.y, 0x01000100u, sq, false);
        si = __builtin_amdgcn_udot4(s.z, 0x00010001u, si, false);
        sq = __builtin_amdgcn_udot4(s.z, 0x01000100u, sq, false);
        si = __builtin_amdgcn_udot4(s.w, 0x00010001u, si, false);
        sq = __builtin_amdgcn_udot4(s.w, 0x01000100u, sq, false);
        return make_int2((int)si - 8 * 128, (int)sq - 8 * 128);
    } else if constexpr (SRC == SRC_CU8_12) {            // 24 bytes, 8-byte aligned: three 8-byte loads
        const nt_u2* q = reinterpret_cast<const nt_u2*>(src) + g * 3;
        unsigned si = 0, sq = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const nt_u2 s = __builtin_nontemporal_load(q + i);
            si = __builtin_amdgcn_udot4(s.x, 0x00010001u, si, false);
            sq = __builtin_amdgcn_udot4(s.x, 0x01000100u, sq, false);
            si = __builtin_amdgcn_udot4(s.y, 0x00010001u, si, false);
            sq = __builtin_amdgcn_udot4(s.y, 0x01000100u, sq, false);
        }
        return make_int2((int)si - 12 * 128, (int)sq - 12 * 128);
    } else if constexpr (SRC == SRC_CU8_10) {            // 20 bytes, 4-byte aligned: five 4-byte loads
        const unsigned* q = reinterpret_cast<const unsigned*>(src) + g * 5;
        unsigned si = 0, sq = 0;
#pragma unroll
        for (int i = 0; i < 5; ++i) {
            const unsigned s = __builtin_nontemporal_load(q + i);
            si = __builtin_amdgcn_udot4(s, 0x00010001u, si, false);
            sq = __builtin_amdgcn_udot4(s, 0x01000100u, sq, false);
        }
        return make_int2((int)si - 10 * 128, (int)sq - 10 * 128);
    } else {                                             // any factor: R two-byte loads
        const uint16_t* q = reinterpret_cast<const uint16_t*>(src) + g * R;
        unsigned si = 0, sq = 0;
        for (int i = 0; i < R; ++i) {
            const unsigned x = q[i];
            si += x & 0xffu;
            sq += x >> 8;
        }
        return make_int2((int)si - 128 * R, (int)sq - 128 * R);
    }
}

__device__ __forceinline__ float phase_of(int2 s) { return atan2_approx_dev((float)s.y, (float)s.x); }

// ---- the streams evaluated one element at a time from device memory: the tails, by the last workgroup ----
template <int SRC>
__device__ __forceinline__ float phase_at(const ChainParams& p, long g)
{
    return g < 0 ? p.state_in[0] : phase_of(load_sample<SRC>(p.src, g, p.cic_r));
}
template <int SRC>
__device__ __forceinline__ float stage1_at(const ChainParams& p, const Maps& m, long s1)
{
    if (s1 < 0) return p.state_in[11 + s1];
    const long g = m.s1_to_g(s1);
    return fm_limit_dev(phase_at<SRC>(p, g), phase_at<SRC>(p, g - 1));
}
template <int SRC>
__device__ __forceinline__ float stage2_at(const ChainParams& p, const Maps& m, long s2)
{
    if (s2 < 0) return p.state_in[21 + s2];
    const long c = 2 * m.s2_to_w(s2);
    return halfband_dev(stage1_at<SRC>(p, m, c - 5), stage1_at<SRC>(p, m, c), stage1_at<SRC>(p, m, c - 2),
                        stage1_at<SRC>(p, m, c - 4), stage1_at<SRC>(p, m, c - 6), stage1_at<SRC>(p, m, c - 8),
                        stage1_at<SRC>(p, m, c - 10));
}

// state_out: the phase of the last sample, the last ten of the stage-1 stream, the last ten of the stage-2 stream
// (or state_in's, when the second half-band does not run); and the decimated samples behind the last tile's range
// (the odd ends that no audio sample depends on).
template <int SRC, bool RUN2>
__device__ __forceinline__ void write_tails(const ChainParams& p, const Maps& m)
{
    const int tid = threadIdx.x;
    if (tid < 10) {
        p.state_out[1 + tid] = stage1_at<SRC>(p, m, m.nblocks * m.L1 - 10 + tid);
    } else if (tid >= 64 && tid < 74) {
        const int i = tid - 64;
        if constexpr (RUN2) p.state_out[11 + i] = stage2_at<SRC>(p, m, m.nblocks * m.L2 - 10 + i);
        else p.state_out[11 + i] = p.state_in[11 + i];
    } else if (tid == 128) {
        p.state_out[0] = phase_at<SRC>(p, m.nblocks * m.L - 1);
    } else if (tid >= 192 && p.dec) {
        nt_i2* dec = reinterpret_cast<nt_i2*>(p.dec);
        for (long g = tile_range<TILE>(m, p.ntiles - 1).ghi + 1 + (tid - 192); g < m.nblocks * m.L; g += 64) {
            const int2 s = load_sample<SRC>(p.src, g, p.cic_r);
            const nt_i2 o = {s.x, s.y};
            dec[g] = o;
        }
    }
}

template <int SRC, bool RUN2>
__global__ __launch_bounds__(THREADS) void fm_chain_kernel(const ChainParams p)
{
    __shared__ float lds[LDS_FLOATS];
    const Maps m = make_maps(p.block_len, p.nblocks);
    const long t = blockIdx.x;
    if (t == p.ntiles) {
        write_tails<SRC, RUN2>(p, m);
        return;
    }
    const int tid = threadIdx.x;
    const TileRange r = tile_range<TILE>(m, t);
    // decimated samples this tile stores: from its own first to the next tile's first
    const long own_lo = t == 0 ? 0 : r.glo;
    const long own_hi = t + 1 == p.ntiles ? r.ghi + 1 : tile_range<TILE>(m, t + 1).glo;
    nt_i2* dec = reinterpret_cast<nt_i2*>(p.dec);

    if constexpr (!RUN2) {                               // exhausted pool: the tiles only deliver the decimated samples
        if (dec) {
            for (long g = own_lo + tid; g < own_hi; g += THREADS) {
                const int2 s = load_sample<SRC>(p.src, g, p.cic_r);
                const nt_i2 o = {s.x, s.y};
                __builtin_nontemporal_store(o, dec + g);
            }
        }
        return;
    } else {
        float* phase = lds;                              // [np]: phases glo - 1 .. ghi
        float* s1e = lds + PHASE_CAP;                    // stage-1 stream from s1lo (even): even and odd positions
        float* s1o = s1e + S1_HALF;
        float* s2e = lds;                                // stage-2 stream from s2lo (even), over the phases
        float* s2o = s2e + S2_HALF;

        // A. every sample once: all loads of the thread in flight, then the phases
        constexpr int PER = (PHASE_CAP + THREADS - 1) / THREADS;
        int2 smp[PER];
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * THREADS;
            const long g = r.glo - 1 + i;
            smp[k] = make_int2(0, 0);
            if (i < r.np && g >= 0) smp[k] = load_sample<SRC>(p.src, g, p.cic_r);
        }
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            const int i = tid + k * THREADS;
            const long g = r.glo - 1 + i;
            if (i < r.np) {
                phase[i] = g < 0 ? p.state_in[0] : phase_of(smp[k]);
                if (dec && g >= own_lo && g < own_hi) {
                    const nt_i2 o = {smp[k].x, smp[k].y};
                    __builtin_nontemporal_store(o, dec + g);
                }
            }
        }
        __syncthreads();

        // B. the stage-1 stream: first difference and limiter, or the carried delay line in front of sample 0
        const TileMap to_g(r.s1lo < 0 ? 0 : r.s1lo, m.L1, m.L);
        for (int j = tid; j < r.n1; j += THREADS) {
            const long s1 = r.s1lo + j;
            float v;
            if (s1 < 0) {
                v = p.state_in[11 + s1];
            } else {
                const int i = (int)(to_g(s1) - r.glo) + 1;
                v = fm_limit_dev(phase[i], phase[i - 1]);
            }
            (j & 1 ? s1o : s1e)[j >> 1] = v;
        }
        __syncthreads();

        // C. the stage-2 stream: the first half-band at the positions the second one reads.  Output w sits at
        // stage-1 position 2 w = s1lo + 2 k with k = w - wlo + 5: x[2w - 2q] = s1e[k - q], x[2w - 5] = s1o[k - 3].
        const TileMap to_w(r.s2lo < 0 ? 0 : r.s2lo, m.L2, m.half);
        for (int j = tid; j < r.n2; j += THREADS) {
            const long s2 = r.s2lo + j;
            float v;
            if (s2 < 0) {
                v = p.state_in[21 + s2];
            } else {
                const int k = (int)(to_w(s2) - r.wlo) + 5;
                v = halfband_dev(s1o[k - 3], s1e[k], s1e[k - 1], s1e[k - 2], s1e[k - 3], s1e[k - 4], s1e[k - 5]);
            }
            (j & 1 ? s2o : s2e)[j >> 1] = v;
        }
        __syncthreads();

        // D. audio sample a0 + a sits at stage-2 position s2lo + 2 (a + 5)
        for (int a = tid; a < r.na; a += THREADS) {
            const int k = a + 5;
            p.audio[r.a0 + a] =
                halfband_dev(s2o[k - 3], s2e[k], s2e[k - 1], s2e[k - 2], s2e[k - 3], s2e[k - 4], s2e[k - 5]);
        }
    }
}

__global__ __launch_bounds__(64) void fm_state_copy_kernel(const float* __restrict__ in, float* __restrict__ out)
{
    if (threadIdx.x < 21) out[threadIdx.x] = in[threadIdx.x];
}

template <int SRC>
static hipError_t launch_src(const ChainParams& p, bool run_stage2, hipStream_t st)
{
    if (run_stage2)
        hipLaunchKernelGGL((fm_chain_kernel<SRC, true>), dim3((unsigned)(p.ntiles + 1)), dim3(THREADS), 0, st, p);
    else if (p.dec)
        hipLaunchKernelGGL((fm_chain_kernel<SRC, false>), dim3((unsigned)(p.ntiles + 1)), dim3(THREADS), 0, st, p);
    else {                                               // only the state advances: the last workgroup alone
        ChainParams q = p;
        q.ntiles = 0;
        hipLaunchKernelGGL((fm_chain_kernel<SRC, false>), dim3(1), dim3(THREADS), 0, st, q);
    }
    return hipGetLastError();
}

hipError_t launch_chain(const ChainParams& p, bool run_stage2, hipStream_t st)
{
    if (p.cic_r == 0) return launch_src<SRC_CS32>(p, run_stage2, st);
    if (p.cic_r == 8) return launch_src<SRC_CU8_8>(p, run_stage2, st);
    if (p.cic_r == 10) return launch_src<SRC_CU8_10>(p, run_stage2, st);
    if (p.cic_r == 12) return launch_src<SRC_CU8_12>(p, run_stage2, st);
    return launch_src<SRC_CU8_ANY>(p, run_stage2, st);
}

hipError_t launch_state_copy(const float* state_in, float* state_out, hipStream_t st)
{
    hipLaunchKernelGGL(fm_state_copy_kernel, dim3(1), dim3(64), 0, st, state_in, state_out);
    return hipGetLastError();
}

template <int SRC>
static hipError_t prepare_src()
{
    const hipError_t e = load_kernel(&fm_chain_kernel<SRC, true>);
    return e == hipSuccess ? load_kernel(&fm_chain_kernel<SRC, false>) : e;
}

// load_kernel (rtlws_internal.h) for every instantiation: the first launch then makes no other call
hipError_t prepare_chain()
{
    hipError_t e = load_kernel(&fm_state_copy_kernel);
    if (e == hipSuccess) e = prepare_src<SRC_CS32>();
    if (e == hipSuccess) e = prepare_src<SRC_CU8_8>();
    if (e == hipSuccess) e = prepare_src<SRC_CU8_10>();
    if (e == hipSuccess) e = prepare_src<SRC_CU8_12>();
    if (e == hipSuccess) e = prepare_src<SRC_CU8_ANY>();
    return e;
}

}  // namespace fm
}  // namespace rtlws

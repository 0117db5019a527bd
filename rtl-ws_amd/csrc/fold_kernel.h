// fold_kernel.h -- the kernel of include/rtlws_fold.h as a template over its epilogue: fold.hip
// instantiates it for the product; tools/variants/fold_transposed.hip, the measurement's other epilogue, is the only
// other user.
//
// Lanes run along trial periods.  A wavefront owns 64 consecutive periods, one trial and one sub-integration and walks
// that sub-integration's samples in ascending n.  Its histogram is [bin][lane] f32 in LDS at a pitch of 64 dwords: a
// lane's column is its own bank, so the hot loop has no bank conflict whatever the bins are, and no two lanes ever touch
// one address, so the ascending order holds with no synchronisation at all (the kernel has no barrier).  A lane keeps
// its 64-bit phase in two registers, advances it by its step per sample (an add with carry) and takes the bin as the
// high half of (phase >> 32) * nbins (one v_mul_hi_u32).  The sample is the same for all 64 lanes: a tile of 64 samples
// comes with one coalesced load, a lane a sample, and sample j is broadcast with v_readlane at a constant j in an
// unrolled loop; the next tile's load is in flight under the current tile's additions.  The addition is LDS read,
// v_add_f32, LDS write, four samples to a group whose reads are issued together (add_group).  The LDS float add without
// return gives the same bits on gfx950, subnormals included, but took 190 clocks per wavefront instruction when measured
// (DESIGN.md 4.21).  hits is the same loop adding integer ones, in the workgroups of trial 0 only.
#ifndef RTLWS_CSRC_FOLD_KERNEL_H
#define RTLWS_CSRC_FOLD_KERNEL_H

#include <hip/hip_runtime.h>

#include "fold.h"

namespace rtlws {
namespace fold {

__device__ __forceinline__ void clear_column(float* col, int nbins)
{
    for (int b = 0; b < nbins; ++b) col[b * LANES] = 0.0f;
}

// GROUP consecutive samples into the lane's column, COUNT: integer ones in place of the samples.  The addition is LDS
// read, add, write.  A lane's next sample may fall in the bin of its last one, so a read cannot simply be issued ahead of
// the write before it; within a group it is, and the value is forwarded in registers instead: all GROUP words are read
// first, sample g takes the newest sum of an earlier sample of the group that fell on its word, else the word read, and
// the GROUP sums are written in ascending g, so that a word ends with its last sum.  The bits are those of one sample
// at a time; the read latency is paid once per group.
template <bool COUNT> struct Word { using type = float; };
template <> struct Word<true> { using type = unsigned; };

template <bool COUNT, int GROUP>
__device__ __forceinline__ void add_group(float* col, uint64_t& phase, uint64_t step, unsigned nbins, const float (&x)[GROUP])
{
    using T = typename Word<COUNT>::type;
    T* const mine = reinterpret_cast<T*>(col);
    unsigned bin[GROUP];
    T sum[GROUP];
#pragma unroll
    for (int g = 0; g < GROUP; ++g) {
        bin[g] = __umulhi((unsigned)(phase >> 32), nbins);
        asm("" : "+v"(bin[g]));                               // the bin as it is: its word is then one shift-and-add, not a 64-bit product's shift and mask
        phase += step;
    }
#pragma unroll
    for (int g = 0; g < GROUP; ++g) sum[g] = mine[bin[g] * LANES];
#pragma unroll
    for (int g = 0; g < GROUP; ++g) {
        T acc = sum[g];
#pragma unroll
        for (int h = 0; h < g; ++h) acc = bin[h] == bin[g] ? sum[h] : acc;    // ascending h: the newest wins
        if constexpr (COUNT) sum[g] = acc + 1u;
        else sum[g] = acc + x[g];
    }
#pragma unroll
    for (int g = 0; g < GROUP; ++g) mine[bin[g] * LANES] = sum[g];
}

__device__ __forceinline__ float sample_of_lane(float tile, int j)
{
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(tile), j));
}

// The samples series[0 .. len - 1] into the wavefront's columns in ascending n.  No sample at or beyond len is read
__device__ __forceinline__ void fold_samples(float* col, uint64_t phase, uint64_t step, unsigned nbins, const float* series, int len, int lane)
{
    float tile = lane < len ? series[lane] : 0.0f;
    for (int j0 = 0; j0 < len; j0 += TILE) {
        const int cnt = len - j0 < TILE ? len - j0 : TILE;
        float next = 0.0f;
        if (j0 + TILE + lane < len) next = series[j0 + TILE + lane];      // in flight under this tile's additions
        if (cnt == TILE) {
#pragma unroll
            for (int j = 0; j < TILE; j += GROUP) {
                float x[GROUP];
#pragma unroll
                for (int g = 0; g < GROUP; ++g) x[g] = sample_of_lane(tile, j + g);
                add_group<false, GROUP>(col, phase, step, nbins, x);
            }
        } else {
            for (int j = 0; j < cnt; ++j) {
                const float x[1] = {sample_of_lane(tile, j)};
                add_group<false, 1>(col, phase, step, nbins, x);
            }
        }
        tile = next;
    }
}

__device__ __forceinline__ void count_samples(float* col, uint64_t phase, uint64_t step, unsigned nbins, int len)
{
    const float none[GROUP] = {};
    int j = 0;
    for (; j + GROUP <= len; j += GROUP) add_group<true, GROUP>(col, phase, step, nbins, none);
    for (; j < len; ++j) add_group<true, 1>(col, phase, step, nbins, reinterpret_cast<const float(&)[1]>(none));
}

// The epilogue, [bin][lane] -> nbins contiguous words per period, as a policy: store(hist, lane, valid, rows, pitch, nbins)
// writes the columns of the wavefront's first `valid` lanes, hist its histogram, rows the first period's row and pitch
// the words between two periods' rows.  RowReads: every lane reads its own column (no bank conflict) and stores to its
// own period's row, four bins in flight (the form chosen over the transposed read of
// tools/variants/fold_transposed.hip)
struct RowReads {
    template <typename T>
    static __device__ __forceinline__ void store(const float* hist, int lane, int valid, T* rows, long pitch, int nbins)
    {
        if (lane >= valid) return;
        const T* const c = reinterpret_cast<const T*>(hist) + lane;
        T* const row = rows + lane * pitch;
        int b = 0;
        for (; b + 4 <= nbins; b += 4) {
            const T v0 = c[b * LANES], v1 = c[(b + 1) * LANES], v2 = c[(b + 2) * LANES], v3 = c[(b + 3) * LANES];
            row[b] = v0;
            row[b + 1] = v1;
            row[b + 2] = v2;
            row[b + 3] = v3;
        }
        for (; b < nbins; ++b) row[b] = c[b * LANES];
    }
};

template <int WPB, typename Epilogue>
__global__ __launch_bounds__(WPB * LANES) void fold_kernel(const Params p)
{
    extern __shared__ __attribute__((aligned(16))) float lds[];

    const int lane = threadIdx.x & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // workgroup (t, s, g): the groups of one trial and sub-integration side by side, they read the same samples
    const unsigned groups = (unsigned)p.groups, nsub = (unsigned)p.nsub;
    const unsigned g = blockIdx.x % groups, ts = blockIdx.x / groups;
    const long s = (long)(ts % nsub), t = (long)(ts / nsub);
    const int first = (int)(g * WPB + wave) * LANES;           // the wavefront's first period
    if (first >= p.nperiods) return;                          // a whole wavefront behind the table: nothing to do, no barrier to miss
    const int valid = p.nperiods - first < LANES ? p.nperiods - first : LANES;       // lanes behind the table idle along on the last period's
    const int period = lane < valid ? first + lane : p.nperiods - 1;                 // values, and nothing of theirs is stored

    const long n0 = s * p.sub;
    const int len = (int)((n0 + p.sub < p.nsamp ? n0 + p.sub : p.nsamp) - n0);          // this sub-integration's samples: 1 .. sub
    const unsigned nbins = (unsigned)p.nbins;
    const uint64_t step = p.steps[period];
    const uint64_t phase = p.phases[period] + (uint64_t)n0 * step;                      // phase_p(n0), mod 2^64
    float* const hist = lds + wave * (p.nbins * LANES);
    float* const col = hist + lane;
    const long pitch = p.nsub * p.nbins;
    const long rows = first * pitch + s * p.nbins;                                      // of hits; a trial's profiles lie nperiods * pitch apart

    clear_column(col, p.nbins);
    fold_samples(col, phase, step, nbins, p.in + t * p.in_stride + n0, len, lane);
    Epilogue::store(hist, lane, valid, p.prof + t * p.nperiods * pitch + rows, pitch, p.nbins);

    if (t == 0 && p.hits != nullptr) {
        clear_column(col, p.nbins);
        count_samples(col, phase, step, nbins, len);
        Epilogue::store(hist, lane, valid, p.hits + rows, pitch, p.nbins);
    }
}

}  // namespace fold
}  // namespace rtlws
#endif

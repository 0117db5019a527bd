// subdedisp.hip -- the kernels of include/rtlws_subdedisp.h (librtlws_subdedisp.so): the subbands' sums
// of every nominal trial over a waterfall of f32 rows, then every trial over the subband series of its nominal; two
// launches.
//
// Stage 1 is the dedispersion's tile (dedisp.h) over the table of the nominals: the same walk of the row, and at a
// subband's last position every chain's sum goes to the workspace, lanes along time, and begins again at +0.0f.
// Stage 2 has the same shape one level up: a workgroup owns TILE_OUT outputs of up to TRIALS trials of one nominal, the
// windows of that nominal's subband series come into LDS by coalesced loads (they are already contiguous in time), and
// an addition reads tile[subband][n - n0 + d2 - base] at a scalar offset from the plan's table.
#include <hip/hip_runtime.h>

#include "rtlws_internal.h"
#include "subdedisp.h"

namespace rtlws {
namespace subdedisp {

using dedisp::Params;

// the plan's tables through the constant address space: loads at a workgroup-uniform index are scalar loads
template <typename T>
using Constant = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ Constant<T> constant(const T* p) { return (Constant<T>)(p); }

// a position's offsets under the TRIALS chains of a group, and the int2 and int4 of a table as a scalar load gives them
template <int TRIALS> struct Offsets { typedef int type __attribute__((ext_vector_type(TRIALS))); };
template <> struct Offsets<1> { typedef int type; };

// Window row r of a unit, clamped into what the run may read: the rows at or beyond rows_needed are never read, and
// only values at or beyond nmid would have used them
__device__ __forceinline__ const float* window_row(const float* rows, long in_stride, long first, int r, long rows_needed)
{
    const long row = first + r;
    return rows + (row < rows_needed ? row : rows_needed - 1) * in_stride;
}

struct Params1 {
    Params p;              // dedisp.h's, of d1 as a table of nnominal trials: out the workspace, out_stride mid_stride, nout nmid
    int per, nsub;         // positions of a subband, subbands
};

// Stage 1: dedisp.hip's walk (dedisp.h's tile: TILE_OUT values m of TRIALS consecutive nominals, the chunk's window
// transposed through LDS in 16-byte loads along the row, the delays scalar loads) with one difference: at a subband's
// last position, a workgroup-uniform condition that may fall anywhere in a chunk, every chain's acc is stored to its
// series of the workspace, 64 consecutive floats a wavefront, and set back to +0.0f.  dedisp.hip's text is not shared:
// with the epilogue as a parameter its code objects did not stay what they were
template <int TRIALS, bool LONE, bool BIG>
__global__ __launch_bounds__(THREADS) void subdedisp_subband_kernel(const Params1 k)
{
    __shared__ float tile[BIG ? BIG_WORDS : SMALL_WORDS];
    typedef typename Offsets<TRIALS>::type RelT;
    constexpr int DEPTH = 4;                                  // loads of a thread in flight

    const Params& p = k.p;
    const int tid = threadIdx.x;
    const int M = p.nchan, chunk = p.chunk, stride = p.stride;
    const int group = (int)(blockIdx.x % (unsigned)p.ngroups);
    const long n0 = (long)(blockIdx.x / (unsigned)p.ngroups) * TILE_OUT;
    const long rows_needed = p.rows_needed, in_stride = p.in_stride;
    const float* const rows = p.rows;
    const int2* const units = p.units + (long)group * (LONE ? M : M / 4);
    const Constant<RelT> rel = (Constant<RelT>)(constant(p.rel) + (long)group * M * TRIALS);

    float acc[TRIALS];
#pragma unroll
    for (int c = 0; c < TRIALS; ++c) acc[c] = 0.0f;
    tile[chunk * stride + tid] = 0.0f;                        // the column of zeros behind the chunk's: never written again

    // where the sums go: value m of the subband the walk is in, under the group's first nominal; the chains that are
    // nominals of the table, none for a thread at or beyond nmid
    const long nominal_step = (long)k.nsub * p.out_stride;
    float* dst = p.out + (long)group * TRIALS * nominal_step + (n0 + tid);
    const int chains = n0 + tid < p.nout ? p.ntrials - group * TRIALS : 0;
    int border = k.per;                                       // the first position of the next subband

    for (int c0 = 0; c0 < M; c0 += chunk) {
        // 1: the chunk's window, transposed; DEPTH rows of a thread at a time, the last ones of a column repeated
        if constexpr (LONE) {
            const int il = tid & (MAX_CHUNK - 1), i = c0 + il;
            const int2 u = i < M ? units[i] : make_int2(-1, 0);
            if (u.x >= 0) {
                constexpr int STEP = THREADS / MAX_CHUNK;
                const int last = TILE_OUT - 1 + u.y, h = i & 3;
                float* const col = tile + il * stride;
                for (int r0 = tid / MAX_CHUNK; r0 <= last; r0 += DEPTH * STEP) {
                    float4 v[DEPTH];
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) {
                        const int r = r0 + j * STEP < last ? r0 + j * STEP : last;
                        v[j] = *reinterpret_cast<const float4*>(window_row(rows, in_stride, n0 + u.x, r, rows_needed) + (i & ~3));
                    }
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) {
                        const int r = r0 + j * STEP < last ? r0 + j * STEP : last;
                        col[r] = h == 0 ? v[j].x : h == 1 ? v[j].y : h == 2 ? v[j].z : v[j].w;
                    }
                }
            }
        } else {
            const int quads = chunk / 4;                      // 8, 4, 2, 1
            const int ql = tid & (quads - 1), q = c0 / 4 + ql, step = THREADS / quads;
            const int2 u = 4 * q < M ? units[q] : make_int2(-1, 0);
            if (u.x >= 0) {
                const int last = TILE_OUT - 1 + u.y;
                float* const col = tile + 4 * ql * stride;
                for (int r0 = tid / quads; r0 <= last; r0 += DEPTH * step) {
                    float4 v[DEPTH];
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) {
                        const int r = r0 + j * step < last ? r0 + j * step : last;
                        v[j] = *reinterpret_cast<const float4*>(window_row(rows, in_stride, n0 + u.x, r, rows_needed) + 4 * q);
                    }
#pragma unroll
                    for (int j = 0; j < DEPTH; ++j) {
                        const int r = r0 + j * step < last ? r0 + j * step : last;
                        col[r] = v[j].x;
                        col[stride + r] = v[j].y;
                        col[2 * stride + r] = v[j].z;
                        col[3 * stride + r] = v[j].w;
                    }
                }
            }
        }
        __syncthreads();

        // 2: the chunk's terms, ascending, in runs that end where a subband does.  A position's TRIALS reads start at the
        // words of the tile that one scalar load of the plan's table names: its column at the nominal's delay, or for a
        // position the mask leaves out the column of zeros.  acc is never -0 (it starts at +0), so adding +0 leaves
        // every acc as it is, bit for bit, and a subband with nothing kept is stored as +0.0
        const int count = M - c0 < chunk ? M - c0 : chunk;
        const Constant<RelT> words = rel + c0;
        const float* const mine = tile + tid;
        for (int il = 0; il < count;) {
            const int end = border - c0 < count ? border - c0 : count;
#pragma unroll 4
            for (; il < end; ++il) {
                const RelT w = words[il];
                if constexpr (TRIALS == 1) {
                    acc[0] = acc[0] + mine[w];
                } else {
#pragma unroll
                    for (int c = 0; c < TRIALS; ++c) acc[c] = acc[c] + mine[w[c]];
                }
            }
            if (c0 + il == border) {                          // the subband's last position is behind us
#pragma unroll
                for (int c = 0; c < TRIALS; ++c) {
                    if (c < chains) dst[c * nominal_step] = acc[c];
                    acc[c] = 0.0f;
                }
                dst += p.out_stride;
                border += k.per;
            }
        }
        __syncthreads();                                      // the window is read: the tile may be written
    }
}

template <int TRIALS, bool BIG>
__global__ __launch_bounds__(THREADS) void subdedisp_trial_kernel(const Params2 p)
{
    __shared__ float tile[BIG ? BIG_WORDS : SMALL_WORDS];
    typedef typename Offsets<TRIALS>::type RelT;
    typedef Offsets<2>::type Int2;                            // int2 and int4 as a scalar load gives them
    typedef Offsets<4>::type Int4;
    constexpr int DEPTH = 8;                                  // subbands of a thread in flight
    static_assert((BIG_WORDS - TILE_OUT) / MAX_CHUNK < 2 * TILE_OUT, "a column is more than two values a thread");

    const int tid = threadIdx.x;
    const int B = p.nsub, stride = p.stride;
    const int group = (int)(blockIdx.x % (unsigned)p.ngroups);
    const long n0 = (long)(blockIdx.x / (unsigned)p.ngroups) * TILE_OUT;
    const long nmid = p.nmid, mid_stride = p.mid_stride;
    const Int4 g = ((Constant<Int4>)constant(p.groups))[group];                     // {first trial, trials, nominal, 0}
    const float* const series = p.mid + (long)g.z * B * mid_stride;
    const Constant<Int2> units = (Constant<Int2>)constant(p.units) + (long)group * B;
    const Constant<RelT> rel = (Constant<RelT>)(constant(p.rel) + (long)group * B * TRIALS);

    float acc[TRIALS];
#pragma unroll
    for (int k = 0; k < TRIALS; ++k) acc[k] = 0.0f;
    tile[MAX_CHUNK * stride + tid] = 0.0f;                    // the column of zeros behind the chunk's: never written again

    for (int c0 = 0; c0 < B; c0 += MAX_CHUNK) {
        const int count = B - c0 < MAX_CHUNK ? B - c0 : MAX_CHUNK;
        // 1: the chunk's windows, a subband's series along the lanes; the values at or beyond nmid are never read, and
        // only outputs at or beyond nout would have used them.  DEPTH subbands of a thread in flight; a column is TILE_OUT + span < 2 TILE_OUT values, a thread's first always there
        for (int il0 = 0; il0 < count; il0 += DEPTH) {
            float v[DEPTH], w[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                const int il = il0 + j;
                if (il >= count) break;
                const Int2 u = units[c0 + il];
                if (u.x < 0) continue;
                const float* const src = series + (long)(c0 + il) * mid_stride;
                const long m = n0 + u.x + tid;
                v[j] = src[m < nmid ? m : nmid - 1];
                if (tid < u.y) w[j] = src[m + TILE_OUT < nmid ? m + TILE_OUT : nmid - 1];
            }
#pragma unroll
            for (int j = 0; j < DEPTH; ++j) {
                const int il = il0 + j;
                if (il >= count) break;
                const Int2 u = units[c0 + il];
                if (u.x < 0) continue;
                float* const col = tile + il * stride;
                col[tid] = v[j];
                if (tid < u.y) col[tid + TILE_OUT] = w[j];
            }
        }
        __syncthreads();

        // 2: the chunk's terms, ascending; a subband that keeps no position reads the column of zeros, which leaves
        // every acc as it is (acc is never -0)
        const Constant<RelT> words = rel + c0;
        const float* const mine = tile + tid;
#pragma unroll 4
        for (int il = 0; il < count; ++il) {
            const RelT w = words[il];
            if constexpr (TRIALS == 1) {
                acc[0] = acc[0] + mine[w];
            } else {
#pragma unroll
                for (int k = 0; k < TRIALS; ++k) acc[k] = acc[k] + mine[w[k]];
            }
        }
        __syncthreads();                                      // the windows are read: the tile may be written
    }

    const long n = n0 + tid;
    if (n < p.nout) {
#pragma unroll
        for (int k = 0; k < TRIALS; ++k)
            if (k < g.y) p.out[(long)(g.x + k) * p.out_stride + n] = acc[k];
    }
}

// the launch tables: f is handed the instantiation of the stage's form
using TrialCounts = Vals<8, 4, 2, 1>;
static_assert(MAX_TRIALS_PER_BLOCK == 8, "dedisp.h and the launch tables disagree");

template <typename F>
static hipError_t with_stage1(const Layout& l, F&& f)
{
    if (l.lone) return l.trials == 1 && !l.big ? f(&subdedisp_subband_kernel<1, true, false>) : hipErrorInvalidValue;
    return pick(TrialCounts{}, l.trials, [&](auto t) { return pick(Bools{}, l.big != 0, [&](auto b) { return f(&subdedisp_subband_kernel<t, false, b>); }); });
}

template <typename F>
static hipError_t with_stage2(const Layout& l, F&& f)
{
    if (!l.lone || l.chunk != MAX_CHUNK) return hipErrorInvalidValue;
    if (l.trials == 1) return !l.big ? f(&subdedisp_trial_kernel<1, false>) : hipErrorInvalidValue;
    return pick(Vals<8, 4, 2>{}, l.trials, [&](auto t) { return pick(Bools{}, l.big != 0, [&](auto b) { return f(&subdedisp_trial_kernel<t, b>); }); });
}

hipError_t launch_stage1(const Layout& l, const Params& p, int per, int nsub, hipStream_t st)
{
    const long blocks = (p.nout + TILE_OUT - 1) / TILE_OUT * p.ngroups;
    const Params1 kp{p, per, nsub};
    return with_stage1(l, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, kp); });
}

hipError_t launch_stage2(const Layout& l, const Params2& p, hipStream_t st)
{
    const long blocks = (p.nout + TILE_OUT - 1) / TILE_OUT * p.ngroups;
    return with_stage2(l, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_stage1(const Layout& l)
{
    return with_stage1(l, [](auto kernel) { return load_kernel(kernel); });
}

hipError_t prepare_stage2(const Layout& l)
{
    return with_stage2(l, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace subdedisp
}  // namespace rtlws

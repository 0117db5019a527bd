// dedisp.hip -- the kernels of include/rtlws_dedisp.h (librtlws_dedisp.so): every trial of a table of
// per-position delays over a waterfall of f32 rows, one launch.
//
// A workgroup owns TILE_OUT consecutive outputs (one per thread, lanes along time) of TRIALS consecutive trials, whose
// accumulators stay in registers: TRIALS independent chains of additions, each strictly in ascending position.  The
// rows are [time][position] and the sum wants lanes along time, so the row is walked in chunks: the window of rows
// the chunk's positions need under these trials is loaded with 16-byte loads along the row and laid in LDS
// position-major (dedisp.h), after which an addition reads tile[position][n - n0 + delay - base]: consecutive lanes
// consecutive words.  The delays are the same for the whole workgroup: they come as scalar loads from the plan's
// table, and the vector unit spends one address addition and one float addition per term.
#include <hip/hip_runtime.h>

#include "dedisp.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace dedisp {

// the plan's tables through the constant address space: loads at a workgroup-uniform index are scalar loads
template <typename T>
using Constant = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ Constant<T> constant(const T* p) { return (Constant<T>)(p); }

// a position's offsets under the TRIALS trials of a group
template <int TRIALS> struct Offsets { typedef int type __attribute__((ext_vector_type(TRIALS))); };
template <> struct Offsets<1> { typedef int type; };

// Window row r of a unit, clamped into what the run may read: the rows at or beyond rows_needed are never read, and
// only outputs at or beyond nout would have used them
__device__ __forceinline__ const float* window_row(const float* rows, long in_stride, long first, int r, long rows_needed)
{
    const long row = first + r;
    return rows + (row < rows_needed ? row : rows_needed - 1) * in_stride;
}

template <int TRIALS, bool LONE, bool BIG>
__global__ __launch_bounds__(THREADS) void dedisp_kernel(const Params p)
{
    __shared__ float tile[BIG ? BIG_WORDS : SMALL_WORDS];
    typedef typename Offsets<TRIALS>::type RelT;
    constexpr int DEPTH = 4;                                  // loads of a thread in flight

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
    for (int k = 0; k < TRIALS; ++k) acc[k] = 0.0f;
    tile[chunk * stride + tid] = 0.0f;                        // the column of zeros behind the chunk's: never written again

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

        // 2: the chunk's terms, ascending.  A position's TRIALS reads start at the words of the tile that one scalar
        // load of the plan's table names: its column at the trial's delay, or for a position the mask leaves out the
        // column of zeros.  acc is never -0 (it starts at +0), so adding +0 leaves every acc as it is, bit for bit
        const int count = M - c0 < chunk ? M - c0 : chunk;
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
        __syncthreads();                                      // the window is read: the tile may be written
    }

    const long n = n0 + tid;
    if (n < p.nout) {
#pragma unroll
        for (int k = 0; k < TRIALS; ++k) {
            const int t = group * TRIALS + k;
            if (t < p.ntrials) p.out[t * p.out_stride + n] = acc[k];
        }
    }
}

// the launch table: f is handed the instantiation of the plan's form
using TrialCounts = Vals<8, 4, 2, 1>;
static_assert(MAX_TRIALS_PER_BLOCK == 8, "dedisp.h and the launch table disagree");

template <typename F>
static hipError_t with_kernel(const Layout& l, F&& f)
{
    if (l.lone) return l.trials == 1 && !l.big ? f(&dedisp_kernel<1, true, false>) : hipErrorInvalidValue;
    return pick(TrialCounts{}, l.trials, [&](auto t) { return pick(Bools{}, l.big != 0, [&](auto b) { return f(&dedisp_kernel<t, false, b>); }); });
}

hipError_t launch_dedisp(const Layout& l, const Params& p, hipStream_t st)
{
    const long blocks = (p.nout + TILE_OUT - 1) / TILE_OUT * p.ngroups;
    return with_kernel(l, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

// load_kernel (rtlws_internal.h) for the kernel of a form
hipError_t prepare_dedisp(const Layout& l)
{
    return with_kernel(l, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace dedisp
}  // namespace rtlws

// pulse.hip -- the kernel of include/rtlws_pulse.h (librtlws_pulse.so): boxcar sums of every width of a
// table over every trial's series, the largest per segment and where it lies, and the segment's moments, one launch.
//
// A workgroup owns one segment of one trial and walks it in tiles, lanes along n.  A tile's samples are staged in LDS
// with 16-byte loads (level 0) and the levels are built by doubling, P_(l+1)[n] = P_l[n] + P_l[n + 2^l], over the halo
// too, with a barrier between levels.  A width's sum is then its pieces, highest bit first: consecutive lanes read
// consecutive words at an offset that is the same for the whole workgroup, so the pieces' places come as scalar loads
// from the plan's table.  Every thread keeps a (best, at) pair per width in registers; behind the last tile the pairs
// are reduced across the workgroup (the greater value, among equal values the smaller n) and the moments in the
// header's tree.  Plain loads and stores only.
#include <hip/hip_runtime.h>

#include "pulse.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace pulse {

// the plan's table through the constant address space: loads at a workgroup-uniform index are scalar loads
template <typename T>
using Constant = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ Constant<T> constant(const T* p) { return (Constant<T>)(p); }

// Samples i .. i + 3 of a series, i a multiple of 4 and below `need`: no sample at or beyond `need` is read (the last
// one before it stands in; only words behind the tile's halo get it)
__device__ __forceinline__ float4 load_quad(const float* series, long i, long need)
{
    if (i + 3 < need) return *reinterpret_cast<const float4*>(series + i);
    const long last = need - 1;
    return make_float4(series[i], series[i + 1 < last ? i + 1 : last], series[i + 2 < last ? i + 2 : last], series[last]);
}

// the pair that wins: the greater value; among equal values the smaller n.  A pair that saw nothing is (-Inf, -1)
__device__ __forceinline__ void take_better(float& b, int& a, float ob, int oa)
{
    const bool take = (ob > b) | ((ob == b) & (oa < a));      // selects, no branches
    b = take ? ob : b;
    a = take ? oa : a;
}

template <int WORDS, int U>
__global__ __launch_bounds__(THREADS) void pulse_kernel(const Params p)
{
    __shared__ __attribute__((aligned(16))) float lds[WORDS];
    constexpr int DEPTH = 4;                                  // loads of a thread in flight

    const int tid = threadIdx.x;
    const Constant<int> table = constant(p.table);
    constexpr int T = U * THREADS;                           // tile_out
    const int nw = p.nwidths, top = p.top, halo = p.w_max - 1;
    const long s = (long)(blockIdx.x % (unsigned)p.nseg), t = (long)(blockIdx.x / (unsigned)p.nseg);
    const long seg0 = s * p.seg, need = p.need;
    const int len = (int)((seg0 + p.seg < p.nout ? seg0 + p.seg : p.nout) - seg0);        // this segment's outputs: 1 .. seg
    const float* const series = p.in + t * p.in_stride;
    const bool moments = p.mom != nullptr;

    float best[MAX_WIDTHS];
    int at[MAX_WIDTHS];
#pragma unroll
    for (int k = 0; k < MAX_WIDTHS; ++k) {
        best[k] = -__builtin_inff();
        at[k] = -1;
    }
    double q1 = 0.0, q2 = 0.0;

    for (int j0 = 0; j0 < len; j0 += T) {
        const int cnt = len - j0 < T ? len - j0 : T;          // outputs of this tile
        const long n0 = seg0 + j0;

        // 1: level 0, the tile's samples and its halo: n0 .. n0 + cnt + w_max - 2 (all below `need`), whole quads
        const int len0 = cnt + halo, quads = (len0 + 3) >> 2;
        float* const row0 = lds + table[LEVEL_ROW];
        for (int q0 = tid; q0 < quads; q0 += DEPTH * THREADS) {
            float4 v[DEPTH];
#pragma unroll
            for (int j = 0; j < DEPTH; ++j)
                if (q0 + j * THREADS < quads) v[j] = load_quad(series, n0 + 4 * (q0 + j * THREADS), need);
#pragma unroll
            for (int j = 0; j < DEPTH; ++j)
                if (q0 + j * THREADS < quads) *reinterpret_cast<float4*>(row0 + 4 * (q0 + j * THREADS)) = v[j];
        }
        __syncthreads();

        // 2: the moments of the tile's own samples: j0 is a multiple of 256, so thread r holds residue class r
        if (moments)
            for (int i = tid; i < cnt; i += THREADS) {
                const double x = (double)row0[i];
                q1 = q1 + x;
                q2 = q2 + x * x;                              // the product is exact: contracted or not, one rounding
            }

        // 3: the levels by doubling; level l holds len0 - (2^l - 1) entries.  The barrier also keeps a row that two
        // levels use in turn from being written while the level before last is still read
        int entries = len0;
        for (int l = 0; l < top; ++l) {
            const float* const src = lds + table[LEVEL_ROW + l];
            float* const dst = lds + table[LEVEL_ROW + l + 1];
            const int step = 1 << l;
            entries -= step;
            for (int i = tid; i < entries; i += THREADS) dst[i] = src[i] + src[i + step];
            __syncthreads();
        }

        // 4: every width's sum of every output of the tile, its pieces highest bit first, into the thread's pairs
        // (a thread's outputs tid, tid + 256, .. side by side: one scalar load of a piece's place serves them all; an
        // output at or beyond cnt reads words of its row that no output uses, and is not compared)
        const float* const mine = lds + tid;
        int widths_here = nw;                                 // opaque per tile: sixteen comparisons with it held across
        asm volatile("" : "+s"(widths_here));                 // the tiles would take thirty-two scalar registers
#pragma unroll
        for (int k = 0; k < MAX_WIDTHS; ++k) {
            if (k >= widths_here) continue;
            const int first = table[FIRST + k], end = table[FIRST + k + 1];
            float b[U];
            {
                const int place = table[first];
#pragma unroll
                for (int u = 0; u < U; ++u) b[u] = mine[place + u * THREADS];
            }
            for (int j = first + 1; j < end; ++j) {
                const int place = table[j];
#pragma unroll
                for (int u = 0; u < U; ++u) b[u] = b[u] + mine[place + u * THREADS];
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
            {                                                 // strict: NaN never wins, the first of equal values stays
                const bool take = (tid + u * THREADS < cnt) & (b[u] > best[k]);
                best[k] = take ? b[u] : best[k];
                at[k] = take ? (int)n0 + tid + u * THREADS : at[k];
            }
        }
        __syncthreads();                                      // the rows are read: they may be written
    }

    // 5: the pairs across the workgroup: the lanes of a wavefront, then the four wavefronts through LDS
    float* const wave_best = lds + 4 * THREADS;
    int* const wave_at = reinterpret_cast<int*>(wave_best + MAX_WIDTHS * (THREADS / 64));
#pragma unroll
    for (int k = 0; k < MAX_WIDTHS; ++k) {                    // a width the table does not have: (-Inf, -1), never stored
        float b = best[k];
        int a = at[k];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const float ob = __shfl_down(b, d);
            const int oa = __shfl_down(a, d);
            take_better(b, a, ob, oa);                        // a lane whose partner lies outside the wavefront gets itself
        }
        if ((tid & 63) == 0) {
            wave_best[k * (THREADS / 64) + (tid >> 6)] = b;
            wave_at[k * (THREADS / 64) + (tid >> 6)] = a;
        }
    }
    // 6: the moments in the header's tree: q[i] += q[i + h], h = 128 .. 1
    double* const tree = reinterpret_cast<double*>(lds);
    if (moments) {
        tree[tid] = q1;
        tree[THREADS + tid] = q2;
        for (int h = THREADS / 2; h >= 1; h >>= 1) {
            __syncthreads();
            if (tid < h) {
                tree[tid] = tree[tid] + tree[tid + h];
                tree[THREADS + tid] = tree[THREADS + tid] + tree[THREADS + tid + h];
            }
        }
    }
    __syncthreads();
    if (tid < nw) {
        float b = wave_best[tid * (THREADS / 64)];
        int a = wave_at[tid * (THREADS / 64)];
#pragma unroll
        for (int w = 1; w < THREADS / 64; ++w) take_better(b, a, wave_best[tid * (THREADS / 64) + w], wave_at[tid * (THREADS / 64) + w]);
        const long o = (t * nw + tid) * p.nseg + s;
        p.peak[o] = b;
        p.at[o] = a;
    }
    if (moments && tid == 0) {
        double* const m = p.mom + (t * p.nseg + s) * 2;
        m[0] = tree[0];
        m[1] = tree[THREADS];
    }
}

// The launch table: f is handed the instantiation of the plan's tile and LDS.  A tile below 1024 is one whose rows at
// twice the tile pass 64 KiB, so its own rows pass 32 KiB: the largest LDS
using LdsSizes = Vals<0, 1, 2>;
static_assert(MAX_TILE == 4 * THREADS && MIN_TILE == THREADS, "pulse.h and the launch table disagree");

template <typename F>
static hipError_t with_kernel(const Layout& l, F&& f)
{
    if (l.tile_out == MAX_TILE) return pick(LdsSizes{}, l.lds, [&](auto i) { return f(&pulse_kernel<LDS_WORDS[i], 4>); });
    if (l.lds != 2) return hipErrorInvalidValue;
    return l.tile_out == 2 * THREADS ? f(&pulse_kernel<LDS_WORDS[2], 2>) : f(&pulse_kernel<LDS_WORDS[2], 1>);
}

hipError_t launch_pulse(const Layout& l, const Params& p, int ntrials, hipStream_t st)
{
    const long blocks = (long)ntrials * p.nseg;
    return with_kernel(l, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

// load_kernel (rtlws_internal.h) for the kernel of a layout
hipError_t prepare_pulse(const Layout& l)
{
    return with_kernel(l, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace pulse
}  // namespace rtlws

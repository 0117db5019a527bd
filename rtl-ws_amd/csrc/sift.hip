// sift.hip -- the kernels of include/rtlws_sift.h (librtlws_sift.so): the peaks of a single-pulse search
// scored and reduced over the widths, the local maxima of the (trial, segment) plane above a threshold, and those in
// ascending (segment, trial) order as a list; three launches.
//
// Scoring: one thread an event, consecutive lanes consecutive segments, so the loads of a width's peaks are 4 bytes a
// lane and those of the moments 16; the widths come as scalar loads from the plan's table, the loop over them keeps its
// best in registers.  The places are not read here: the list launch reads the place of a candidate's width alone.
// This unit is compiled without contraction: mean * mean and w * mean are roundings of their own (the header's
// definition, rtlws_pulse_snr's operations).
// The box: a tile of the scores with its halo in LDS, NaN outside the plane (no comparison with NaN holds, and no score
// is NaN); a thread walks the box only of an event at or above the threshold.  A candidate's mark goes into the event's
// own word of the workspace, the tile's counts by segment and its two totals behind the planes.
// The list: the position of a candidate is the sum of the counts before it in (segment, trial) order, which every
// workgroup adds up for itself from what the launch before left: nobody waits for anybody, and no sum depends on an order.
#include <hip/hip_runtime.h>

#include "rtlws_internal.h"
#include "sift.h"

namespace rtlws {
namespace sift {

// the plan's table through the constant address space: loads at a workgroup-uniform index are scalar loads
template <typename T>
using Constant = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ Constant<T> constant(const T* p) { return (Constant<T>)(p); }

constexpr float NEG_INF = -__builtin_inff();

// a segment's two moments in one load; d_mom is held to 8 bytes, not to 16
typedef double Moments __attribute__((ext_vector_type(2), aligned(8)));

__global__ __launch_bounds__(THREADS) void sift_score_kernel(const Params p)
{
    constexpr int DEPTH = 4;                                  // widths of a thread in flight
    const unsigned events = (unsigned)p.T * (unsigned)p.S;
    const unsigned e = blockIdx.x * THREADS + threadIdx.x;
    if (e >= events) return;
    const Constant<double> widths = constant(p.widths);
    const int K = p.K;
    const long S = p.S;
    const unsigned t = e / (unsigned)p.S, s = e - t * (unsigned)p.S;
    const long left = p.nout - (long)s * p.seg;
    const long len = left < p.seg ? left : p.seg;

    const Moments q = reinterpret_cast<const Moments*>(p.mom)[e];
    const double count = (double)len;
    const double mean = q.x / count;
    const double var = q.y / count - mean * mean;
    const bool valid = len >= 2 && var > 0.0;

    const float* const peak = p.peak + ((long)t * K * S + s);
    float best = NEG_INF;
    int best_k = 0;
    for (int k0 = 0; k0 < K; k0 += DEPTH) {
        float pk[DEPTH];
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) pk[j] = peak[(k0 + j < K ? k0 + j : K - 1) * S];        // behind the last width: the last one again, not used
#pragma unroll
        for (int j = 0; j < DEPTH; ++j) {
            const int k = k0 + j;
            if (k >= K) break;
            const double w = widths[k];
            const double snr = ((double)pk[j] - w * mean) / __builtin_sqrt(w * var);
            const float sc = (float)snr;
            const bool ok = valid && pk[j] > NEG_INF && sc == sc;        // pk > -Inf: neither -Inf nor NaN
            const float score = ok ? sc : NEG_INF;
            if (score > best) best = score, best_k = k;
        }
    }
    p.score[e] = best;
    p.kword[e] = best_k;
    if (p.d_score) p.d_score[e] = best;
    if (p.d_k) p.d_k[e] = best_k;
}

// the sums of a, b (and c) over the workgroup, in every thread; `part` is [..][THREADS / 64] of LDS, free again behind the call
template <int N>
__device__ __forceinline__ void block_sums(int (&v)[N], int (*part)[THREADS / 64])
{
#pragma unroll
    for (int i = 0; i < N; ++i) {
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) v[i] += __shfl_xor(v[i], m, 64);
    }
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int i = 0; i < N; ++i) part[i][wave] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = (part[i][0] + part[i][1]) + (part[i][2] + part[i][3]);
    __syncthreads();
}
static_assert(THREADS == 256, "block_sums adds four wavefronts");

__global__ __launch_bounds__(THREADS) void sift_box_kernel(const Params p)
{
    __shared__ BoxLds lds;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = p.T, S = p.S, rt = p.rt, rs = p.rs;
    const int tb = (int)(blockIdx.x % (unsigned)p.ntb), sb = (int)(blockIdx.x / (unsigned)p.ntb);
    const int t0 = tb * TILE_T, s0 = sb * TILE_S;
    const float thr = p.threshold;

    // the tile and its halo, a row a wavefront, lanes along s
    const int rows = TILE_T + 2 * rt, cols = TILE_S + 2 * rs;
    for (int r = wave; r < rows; r += THREADS / 64) {
        const int t = t0 - rt + r;
        for (int c = lane; c < cols; c += 64) {
            const int s = s0 - rs + c;
            const bool inside = t >= 0 && t < T && s >= 0 && s < S;
            lds.tile[r * LDS_STRIDE + c] = inside ? p.score[(long)t * S + s] : __builtin_nanf("");
        }
    }
    __syncthreads();

    const int c = lane, s = s0 + c;
    int sums[2] = {0, 0};                                     // candidates, events at or above the threshold
    for (int i = 0; i < ROWS_PER_THREAD; ++i) {
        const int r = wave * ROWS_PER_THREAD + i, t = t0 + r;
        if (t >= T || s >= S) break;
        const float* const centre = lds.tile + (r + rt) * LDS_STRIDE + (c + rs);
        const float v = *centre;
        if (!(v >= thr)) continue;
        ++sums[1];
        bool beaten = false;
        int members = 0, lo = t, hi = t;
        for (int dt = -rt; dt <= rt; ++dt) {
            const float* const row = centre + dt * LDS_STRIDE;
            bool any = false;
            for (int ds = -rs; ds <= rs; ++ds) {
                const float u = row[ds];
                const bool member = u >= thr;
                members += member;
                any |= member;
                beaten |= u > v || (u == v && (dt < 0 || (dt == 0 && ds < 0)));
            }
            if (any) {
                lo = t + dt < lo ? t + dt : lo;
                hi = t + dt > hi ? t + dt : hi;
            }
        }
        if (!beaten) {
            ++sums[0];
            const long e = (long)t * S + s;
            p.kword[e] = (p.kword[e] & K_MASK) | CAND_BIT | members << MEMBERS_SHIFT | (t - lo) << LO_SHIFT | (hi - t) << HI_SHIFT;
        }
    }
    lds.cnt[wave][c] = sums[0];
    block_sums(sums, lds.part);                               // its first barrier is behind the store above
    if (wave == 0) p.cc[(long)blockIdx.x * TILE_S + c] = (lds.cnt[0][c] + lds.cnt[1][c]) + (lds.cnt[2][c] + lds.cnt[3][c]);
    if (tid == 0) p.tot[blockIdx.x] = make_int2(sums[0], sums[1]);
}

__global__ __launch_bounds__(THREADS) void sift_list_kernel(const Params p)
{
    __shared__ ListLds lds;
    const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
    const int T = p.T, S = p.S, ntb = p.ntb;
    const int ntiles = ntb * p.nsb;
    const int tb = (int)(blockIdx.x % (unsigned)ntb), sb = (int)(blockIdx.x / (unsigned)ntb);
    const bool last = (int)blockIdx.x == ntiles - 1;
    const int own = p.tot[blockIdx.x].x;
    if (own == 0 && !last) return;                            // the same for the whole workgroup

    // the candidates of the tiles before this block of segments, in blocks of SCAN_BLOCK totals; the last workgroup adds
    // up every tile's two totals as well, for d_count
    const int before = sb * ntb, upto = last ? ntiles : before;
    int sums[3] = {0, 0, 0};
    for (int i0 = 0; i0 < upto; i0 += SCAN_BLOCK) {
        const int i = i0 + tid;
        if (i < upto) {
            const int2 v = p.tot[i];
            sums[0] += i < before ? v.x : 0;
            sums[1] += v.x;
            sums[2] += v.y;
        }
    }
    block_sums(sums, lds.part);
    if (last && tid == 0) p.count[0] = sums[1], p.count[1] = sums[2];
    if (own == 0) return;
    const int base = sums[0];

    // segment c of this block of segments: the candidates of all its tiles, and of the tiles before this one
    const int32_t* const cc = p.cc + (long)before * TILE_S + c;
    int all = 0, above = 0;
    for (int j = g; j < ntb; j += ROW_GROUPS) {
        const int v = cc[(long)j * TILE_S];
        all += v;
        above += j < tb ? v : 0;
    }
    // this tile's own: the words of the thread's events
    const int t0 = tb * TILE_T + g * ROWS_PER_THREAD, s = sb * TILE_S + c;
    int word[ROWS_PER_THREAD];
    int mine = 0;
#pragma unroll
    for (int i = 0; i < ROWS_PER_THREAD; ++i) {
        word[i] = t0 + i < T && s < S ? p.kword[(long)(t0 + i) * S + s] : 0;
        mine += (word[i] & CAND_BIT) != 0;
    }
    lds.n[0][g][c] = above;
    lds.n[1][g][c] = all;
    lds.n[2][g][c] = mine;
    __syncthreads();
    if (g == 0) {
        int first = base;                                     // the segments before c of this block, over all their tiles
        for (int j = 0; j < c; ++j) first += (lds.n[1][0][j] + lds.n[1][1][j]) + (lds.n[1][2][j] + lds.n[1][3][j]);
        lds.off[c] = first + (lds.n[0][0][c] + lds.n[0][1][c]) + (lds.n[0][2][c] + lds.n[0][3][c]);
    }
    __syncthreads();
    int at = lds.off[c];
    for (int j = 0; j < g; ++j) at += lds.n[2][j][c];
    if (mine == 0) return;
#pragma unroll
    for (int i = 0; i < ROWS_PER_THREAD; ++i) {
        const int w = word[i];
        if (!(w & CAND_BIT)) continue;
        const int idx = at++;
        if (idx >= p.max_cand) continue;
        const int t = t0 + i, k = w & K_MASK;
        const long src = ((long)t * p.K + k) * S + s;
        const float score = p.score[(long)t * S + s];
        uint4 a, b;
        a.x = (unsigned)t, a.y = (unsigned)s, a.z = (unsigned)k, a.w = (unsigned)(score > NEG_INF ? p.at[src] : -1);       // no width scored: (-Inf, 0, -1)
        b.x = __float_as_uint(score);
        b.y = __float_as_uint(p.peak[src]);
        b.z = (unsigned)(w >> MEMBERS_SHIFT & MEMBERS_MASK);
        b.w = (unsigned)(t + (w >> HI_SHIFT & SPAN_MASK)) << 16 | (unsigned)(t - (w >> LO_SHIFT & SPAN_MASK));
        uint4* const dst = reinterpret_cast<uint4*>(p.cand + (long)idx * CAND_WORDS);
        dst[0] = a;
        dst[1] = b;
    }
}
static_assert(sizeof(BoxLds) <= 64 * 1024 && sizeof(ListLds) <= 64 * 1024 && ROW_GROUPS == 4, "static LDS, four row groups");

// the launch table: three kernels, no instantiations; f is handed each in turn until one fails
template <typename F>
static hipError_t with_kernels(F&& f)
{
    hipError_t err = f(&sift_score_kernel, 0);
    if (err == hipSuccess) err = f(&sift_box_kernel, 1);
    return err == hipSuccess ? f(&sift_list_kernel, 2) : err;
}

hipError_t launch_sift(const Params& p, hipStream_t st)
{
    const long events = (long)p.T * p.S, tiles = (long)p.ntb * p.nsb;
    return with_kernels([&](auto kernel, int which) {
        return launch(kernel, dim3((unsigned)(which == 0 ? (events + THREADS - 1) / THREADS : tiles)), dim3(THREADS), 0, st, p);
    });
}

hipError_t prepare_sift()
{
    return with_kernels([](auto kernel, int) { return load_kernel(kernel); });
}

}  // namespace sift
}  // namespace rtlws

// clean.hip -- the kernels of include/rtlws_clean.h (librtlws_clean.so).  Built with -ffp-contract=off:
// var and v are two roundings each.
//
// Stage 1, the statistics.  Lanes run along channels, a lane four neighbouring channels behind one 16-byte load, so a
// wavefront takes 1 KiB of a row.  A workgroup has eight wavefronts, one per residue class of the row index in the
// window; a wavefront walks its rows in ascending k with UNROLL loads in flight and keeps the eight f64 sums of its four
// channels in registers.  The eight partial pairs of a channel meet in LDS [residue][sum][channel] and one thread per
// channel adds them in the tree's order, forms mu, var and sd and writes (mu, sd) to the workspace, sd = -1 where the
// channel is not valid.
//
// Stage 2, the flags.  One workgroup a block.  A thread holds up to four channels' (mu, sd) in registers; the keys of a
// median (invalid channels +Inf, behind the valid ones once sorted) go through a bitonic sort in LDS: the lists of mu and
// of sd side by side in the same steps, then the two lists of deviations -- two rounds of barriers, not four.
// Counts are ballots added in a fixed order: no atomics.  The thread that read a cell writes (m, r, keep) over it.
//
// Stage 3, the rows.  A workgroup stays inside one block; a thread keeps (m, r, keep) of its four channels in registers
// over its rows, and a row's four v between the tree and the subtraction, so a row is read once and written once.  The
// tree's levels below 64 lanes are cross-lane reads inside a wavefront; the levels above, where a row takes several
// wavefronts, are one LDS round trip a row: every wavefront of the row reads the others' 64 partial sums and adds them
// in the tree's order itself, which costs one barrier a row over two buffers used in turn.
#include <hip/hip_runtime.h>

#include "clean.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace clean {

__device__ __forceinline__ bool finite64(double x) { return __builtin_fabs(x) < __builtin_inf(); }
__device__ __forceinline__ bool finite32(float x) { return __builtin_fabsf(x) < __builtin_inff(); }

__global__ __launch_bounds__(STATS_THREADS) void clean_stats_kernel(const StatsParams p)
{
    extern __shared__ __attribute__((aligned(16))) double part[];           // [RES][2][GROUP]

    const int tid = threadIdx.x, lane = tid & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const unsigned groups = (unsigned)p.groups;
    const long b = (long)(blockIdx.x / groups);
    const int first = (int)(blockIdx.x % groups) * GROUP;         // the workgroup's first channel
    const int c0 = first + 4 * lane;
    const int B = p.block_rows;
    const long j0 = b * B < p.nrows - B ? b * B : p.nrows - B;     // the last block looks back

    double q1[4] = {0.0, 0.0, 0.0, 0.0}, q2[4] = {0.0, 0.0, 0.0, 0.0};
    if (c0 < p.nchan) {
        const long stride = p.in_stride * RES;
        const float* src = p.rows + (j0 + wave) * p.in_stride + c0;
        const int count = (B - wave + RES - 1) / RES;             // this residue's rows: k = wave, wave + RES, ..
        int n = 0;
        for (; n + UNROLL <= count; n += UNROLL) {
            float4 x[UNROLL];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) x[u] = *reinterpret_cast<const float4*>(src + u * stride);
            src += UNROLL * stride;
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) {
                const double d[4] = {(double)x[u].x, (double)x[u].y, (double)x[u].z, (double)x[u].w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    q1[e] = q1[e] + d[e];
                    q2[e] = q2[e] + d[e] * d[e];
                }
            }
        }
        for (; n < count; ++n) {
            const float4 x = *reinterpret_cast<const float4*>(src);
            src += stride;
            const double d[4] = {(double)x.x, (double)x.y, (double)x.z, (double)x.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                q1[e] = q1[e] + d[e];
                q2[e] = q2[e] + d[e] * d[e];
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        part[(wave * 2 + 0) * GROUP + 4 * lane + e] = q1[e];
        part[(wave * 2 + 1) * GROUP + 4 * lane + e] = q2[e];
    }
    __syncthreads();
    const int c = first + tid;
    if (tid < GROUP && c < p.nchan) {
        double s[2];
#pragma unroll
        for (int which = 0; which < 2; ++which) {
            double q[RES];
#pragma unroll
            for (int r = 0; r < RES; ++r) q[r] = part[(r * 2 + which) * GROUP + tid];
#pragma unroll
            for (int h = RES / 2; h >= 1; h >>= 1)
#pragma unroll
                for (int r = 0; r < h; ++r) q[r] = q[r] + q[r + h];
            s[which] = q[0];
        }
        const double mu = s[0] / (double)B;
        const double var = s[1] / (double)B - mu * mu;
        const double sd = __builtin_sqrt(var);
        const float r = (float)(1.0 / sd);
        const bool valid = finite64(s[0]) && finite64(s[1]) && var > 0.0 && finite32(r);
        Cell cell;
        cell.mu = mu;
        cell.sd = valid ? sd : -1.0;
        p.cells[b * p.nchan + c] = cell;
    }
}

// ascending bitonic sort of each of the `sets` lists key[s * len .. s * len + len - 1] (len a power of two), all in the same
// steps, by the whole workgroup; ends behind a barrier
__device__ __forceinline__ void sort_keys(double* key, int len, int sets, int tid, int threads)
{
    __syncthreads();                                              // the keys are in place
    for (int k = 2; k <= len; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int idx = tid; idx < len / 2; idx += threads) {
                const int i = ((idx & ~(j - 1)) << 1) | (idx & (j - 1)), l = i | j;
                const bool up = (i & k) == 0;
                for (int s = 0; s < sets; ++s) {
                    double* const list = key + s * len;
                    const double a = list[i], c = list[l];
                    if ((a > c) == up) {
                        list[i] = c;
                        list[l] = a;
                    }
                }
            }
            __syncthreads();
        }
    }
}

// how many of the workgroup's flags are set: a ballot per register, the wavefronts' counts added in ascending order
__device__ __forceinline__ int count_flags(const bool (&flag)[FLAG_PER_THREAD], int* counts, int tid, int threads)
{
    int mine = 0;
#pragma unroll
    for (int e = 0; e < FLAG_PER_THREAD; ++e) mine += __popcll(__ballot(flag[e]));
    __syncthreads();                                              // the counts of an earlier call have been read
    if ((tid & (LANES - 1)) == 0) counts[tid >> 6] = mine;
    __syncthreads();
    int total = 0;
    for (int w = 0; w < threads / LANES; ++w) total += counts[w];
    return total;
}

__global__ __launch_bounds__(1024) void clean_flags_kernel(const FlagParams p)
{
    extern __shared__ __attribute__((aligned(16))) double key[];
    const int tid = threadIdx.x, threads = blockDim.x;
    const int M = p.nchan, len = sort_len(M);
    int* const counts = reinterpret_cast<int*>(key + 2 * len);
    const long b = blockIdx.x;
    Cell* const cells = p.cells + b * M;
    const double inf = __builtin_inf();

    double mu[FLAG_PER_THREAD], sd[FLAG_PER_THREAD];
    bool valid[FLAG_PER_THREAD];
#pragma unroll
    for (int e = 0; e < FLAG_PER_THREAD; ++e) {
        const int i = tid + e * threads;
        const bool in = i < M;
        const Cell cell = in ? cells[i] : Cell{0.0, -1.0};
        mu[e] = cell.mu;
        sd[e] = cell.sd;
        valid[e] = in && p.mask[in ? i : 0] != 0 && cell.sd > 0.0;
    }
    const int nvalid = count_flags(valid, counts, tid, threads);

    // the medians and the MADs of the tests that are made: the lists of both tests sorted in the same steps, mu's first
    double dmu[FLAG_PER_THREAD] = {0.0, 0.0, 0.0, 0.0}, dsd[FLAG_PER_THREAD] = {0.0, 0.0, 0.0, 0.0};
    double mad_mu = 0.0, mad_sd = 0.0;
    const bool test_mean = p.t_mean != inf, test_sigma = p.t_sigma != inf;
    const int sets = (test_mean ? 1 : 0) + (test_sigma ? 1 : 0);
    if (nvalid > 0 && sets > 0) {
        double* const key_mu = key;
        double* const key_sd = key + (test_mean ? len : 0);
        const int mid = (nvalid - 1) / 2;
#pragma unroll
        for (int e = 0; e < FLAG_PER_THREAD; ++e) {
            const int i = tid + e * threads;
            if (i < len && test_mean) key_mu[i] = valid[e] ? mu[e] : inf;
            if (i < len && test_sigma) key_sd[i] = valid[e] ? sd[e] : inf;
        }
        sort_keys(key, len, sets, tid, threads);
        const double med_mu = key_mu[mid], med_sd = key_sd[mid];
        __syncthreads();                                          // every thread has the medians: the keys may go
#pragma unroll
        for (int e = 0; e < FLAG_PER_THREAD; ++e) {
            const int i = tid + e * threads;
            dmu[e] = __builtin_fabs(mu[e] - med_mu);
            dsd[e] = __builtin_fabs(sd[e] - med_sd);
            if (i < len && test_mean) key_mu[i] = valid[e] ? dmu[e] : inf;
            if (i < len && test_sigma) key_sd[i] = valid[e] ? dsd[e] : inf;
        }
        sort_keys(key, len, sets, tid, threads);
        mad_mu = key_mu[mid];
        mad_sd = key_sd[mid];
    }
    const double top_mu = p.t_mean * mad_mu, top_sd = p.t_sigma * mad_sd;

    bool keep[FLAG_PER_THREAD];
#pragma unroll
    for (int e = 0; e < FLAG_PER_THREAD; ++e) keep[e] = valid[e] && (!test_mean || dmu[e] <= top_mu) && (!test_sigma || dsd[e] <= top_sd);
    const int nkept = count_flags(keep, counts, tid, threads);

#pragma unroll
    for (int e = 0; e < FLAG_PER_THREAD; ++e) {
        const int i = tid + e * threads;
        if (i < M) {
            // valid: sd > 0 and (float)(1 / sd) is finite, as stage 1 found
            Flagged f;
            f.m = valid[e] ? (float)mu[e] : 0.0f;
            f.r = valid[e] ? (float)(1.0 / sd[e]) : 0.0f;
            f.keep = keep[e] ? 1 : 0;
            f.unused = 0;
            *reinterpret_cast<Flagged*>(cells + i) = f;
            if (p.keep != nullptr) p.keep[b * M + i] = keep[e] ? 1 : 0;
            if (p.stats != nullptr) {                             // 4-byte aligned: two stores
                p.stats[(b * M + i) * 2] = f.m;
                p.stats[(b * M + i) * 2 + 1] = f.r;
            }
        }
    }
    if (tid == 0) {
        p.ws_nkept[b] = nkept;
        if (p.nkept != nullptr) p.nkept[b] = nkept;
    }
}

// W: the wavefronts a row takes
template <int W>
__global__ __launch_bounds__((W < 4 ? 4 : W) * LANES) void clean_apply_kernel(const ApplyParams p)
{
    extern __shared__ __attribute__((aligned(16))) float sums[];            // W > 1: [2][wavefront][lane]
    constexpr int THREADS = (W < 4 ? 4 : W) * LANES;

    const int tid = threadIdx.x, lane = tid & (LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int row_threads = 1 << p.row_log2, at_once = THREADS >> p.row_log2;
    const int slot = tid >> p.row_log2, q = tid & (row_threads - 1);         // the row among those held at once, the place in it
    const unsigned groups = (unsigned)p.groups;
    const long b = (long)(blockIdx.x / groups);
    const long r0 = b * p.block_rows;
    const long r1 = r0 + p.block_rows < p.nrows ? r0 + p.block_rows : p.nrows;         // the rows the block owns end here
    const long first = r0 + (long)(blockIdx.x % groups) * (at_once * APPLY_ITERS);
    if (first >= r1) return;                                      // the whole workgroup: no barrier is missed

    const int c0 = 4 * q;
    const bool active = c0 < p.nchan;
    float m[4] = {0.0f, 0.0f, 0.0f, 0.0f}, r[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    bool keep[4] = {false, false, false, false};
    if (active) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int4 f = *reinterpret_cast<const int4*>(p.cells + b * p.nchan + c0 + e);          // a Flagged: m, r, keep
            m[e] = __int_as_float(f.x);
            r[e] = __int_as_float(f.y);
            keep[e] = f.z != 0;
        }
    }
    const int nkept = p.ws_nkept[b];
    const float count = (float)nkept;

    long j = first + slot;
    const float* src = p.rows + j * p.in_stride + c0;
    float* dst = p.out + j * p.out_stride + c0;
    const long in_step = (long)at_once * p.in_stride, out_step = (long)at_once * p.out_stride;
    float4 next = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (active && j < r1) next = *reinterpret_cast<const float4*>(src);
    int buf = 0;
    for (int it = 0; it < APPLY_ITERS && first + (long)it * at_once < r1; ++it) {
        const bool live = active && j < r1;
        const float4 x = next;
        src += in_step;
        if (active && j + at_once < r1 && it + 1 < APPLY_ITERS) next = *reinterpret_cast<const float4*>(src);
        const float xs[4] = {x.x, x.y, x.z, x.w};
        float v[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float d = xs[e] - m[e];
            v[e] = live && keep[e] ? d * r[e] : 0.0f;
        }
        if (p.zerodm) {
            float g = ((v[0] + v[1]) + v[2]) + v[3];
            if constexpr (W > 1) {
                float* const mine = sums + buf * THREADS;
                mine[tid] = g;
                __syncthreads();
                float t[W];
                const int base = (wave / W) * W;                  // the row's first wavefront
#pragma unroll
                for (int w = 0; w < W; ++w) t[w] = mine[(base + w) * LANES + lane];
#pragma unroll
                for (int h = W / 2; h >= 1; h >>= 1)
#pragma unroll
                    for (int w = 0; w < h; ++w) t[w] = t[w] + t[w + h];
                g = t[0];
                buf ^= 1;
            }
#pragma unroll
            for (int h = LANES / 2; h >= 1; h >>= 1) {
                const float other = __shfl_down(g, h, LANES);
                g = h < row_threads ? g + other : g;
            }
            const float total = __shfl(g, lane & ~(row_threads - 1), LANES);
            const float z = nkept > 0 ? total / count : 0.0f;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = live && keep[e] ? v[e] - z : 0.0f;
        }
        if (live) *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
        dst += out_step;
        j += at_once;
    }
}

using RowWaves = Vals<1, 2, 4, 8, 16>;

static int log2_of(int pow2)
{
    int l = 0;
    while ((1 << l) < pow2) ++l;
    return l;
}

hipError_t launch_stats(const StatsParams& p, long nblocks, hipStream_t st)
{
    return launch(&clean_stats_kernel, dim3((unsigned)(nblocks * p.groups)), dim3(STATS_THREADS), (size_t)STATS_LDS, st, p);
}

hipError_t launch_flags(const FlagParams& p, long nblocks, hipStream_t st)
{
    return launch(&clean_flags_kernel, dim3((unsigned)nblocks), dim3(flag_threads(p.nchan)), (size_t)flag_lds(p.nchan), st, p);
}

hipError_t launch_apply(const ApplyParams& p, long nblocks, hipStream_t st)
{
    ApplyParams q = p;
    q.row_log2 = log2_of(row_threads(p.nchan));
    return pick(RowWaves{}, row_waves(p.nchan), [&](auto w) {
        return launch(&clean_apply_kernel<decltype(w)::value>, dim3((unsigned)(nblocks * p.groups)), dim3(apply_threads(p.nchan)),
                      (size_t)apply_lds(p.nchan), st, q);
    });
}

// load_kernel (rtlws_internal.h) for the kernels of a channel count
hipError_t prepare(int nchan, int device)
{
    hipError_t err = load_kernel(&clean_stats_kernel);
    if (err == hipSuccess) err = load_kernel(&clean_flags_kernel);
    if (err == hipSuccess) err = lds_opt_in(&clean_flags_kernel, device, (size_t)flag_lds(nchan));        // above 64 KiB from 2052 channels on
    if (err != hipSuccess) return err;
    return pick(RowWaves{}, row_waves(nchan), [&](auto w) { return load_kernel(&clean_apply_kernel<decltype(w)::value>); });
}

}  // namespace clean
}  // namespace rtlws

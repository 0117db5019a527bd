// periodlong.hip -- the kernels of include/rtlws_periodlong.h (librtlws_periodlong.so): the search of
// rtlws_period.h for frames of 2^16 .. 2^22 samples, a four-step transform of the packed series through device memory.
// M = N / 2 = M1 M2 complex points z[j] = y[2 j] + i y[2 j + 1], j = j1 M2 + j2, k = k1 + M1 k2.  Six launches a group
// of trials, a trial at blockIdx.y:
//
//   mean      64 stretches of a trial's samples, one f64 sum each, in a fixed order
//   cols      y = x - mean; the M1-point transforms over j1 of every column j2 in registers (M1 = 256: two radix-16
//             passes around one LDS exchange), the twist e^(-2 pi i k1 j2 / M) from its own once-rounded table, row k1
//             of the workspace
//   rows      the M2-point transform of a row in LDS (row_fft.h), written back in the order of k2
//   untangle  a tile of bins k and the tile of their mirrors M - k through LDS (the rows hold every M1-th bin), the
//             real-input untangling and the square: P in natural order
//   whiten    period.hip's stage 4 over spans of 16384 bins: W over P
//   peaks     period.hip's stage 5 over spans of 16384 bins, W read through the caches
// meet, meet_lanes and the untangling of a pair are period_stages.h's.  Stages 4 and 5 are written out here as they are
// in period.hip, line for line but for a span's first bin: as templates they compile to other instructions (DESIGN.md
// 4.24a), and tests/test_period_family_digest_gpu.py holds the two texts to the same bits.
#include <hip/hip_runtime.h>

#include "period_stages.h"
#include "periodlong.h"
#include "periodlong_front.h"
#include "row_fft.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace periodlong {

namespace stages = period::stages;
using stages::meet;
using stages::meet_lanes;

// ---- mean and cols: periodlong_front.h's text over the series as it lies, the trial of a workgroup at blockIdx.y ----
__device__ __forceinline__ front::Plain series_of(const Params& p) { return front::Plain{p.in + (long)blockIdx.y * p.in_stride}; }

__global__ __launch_bounds__(MEAN_THREADS) void mean_kernel(const Params p) { front::mean(p, series_of(p)); }

__global__ __launch_bounds__(COLS_THREADS) void cols16_kernel(const Params p) { front::cols16(p, series_of(p)); }

__global__ __launch_bounds__(COLS_THREADS) void cols256_kernel(const Params p) { front::cols256(p, series_of(p)); }

// ---- rows: workgroup (k1, trial) transforms row k1 in place; afterwards place k2 of the row holds Z[k1 + M1 k2] ----
template <int LOG2M2>
__global__ __launch_bounds__(rows_threads(LOG2M2)) void rows_kernel(const Params p)
{
    constexpr int M2 = 1 << LOG2M2, T = rows_threads(LOG2M2);
    extern __shared__ float4 lds[];
    float2* const tile = reinterpret_cast<float2*>(lds);
    const int tid = threadIdx.x;
    float2* const row = p.z + ((long)blockIdx.y << (p.log2n - 1)) + (long)blockIdx.x * M2;
#pragma unroll 4
    for (int i = 2 * tid; i < M2; i += 2 * T) {              // i and i + 1 lie in one group of 16
        const float4 v = *reinterpret_cast<const float4*>(row + i);
        float2* const at = tile + rowfft::place(i);
        at[0] = make_float2(v.x, v.y);
        at[1] = make_float2(v.z, v.w);
    }
    __syncthreads();
    rowfft::forward<LOG2M2>(tile, tid, p.tw_row);
#pragma unroll 4
    for (int k2 = tid; k2 < M2; k2 += T) row[k2] = tile[rowfft::place(rowfft::pos<LOG2M2>(k2))];
}

// ---- untangle: workgroup (i, trial) takes bins k = K0 .. K0 + L - 1, K0 = i L < M / 2, and their mirrors M - k ----
// the pair's arithmetic is period_stages.h's untangle and power, the arithmetic of period.hip's stage 3
template <int LOG2M1>
__global__ __launch_bounds__(UNTANGLE_THREADS) void untangle_kernel(const Params p)
{
    constexpr int M1 = 1 << LOG2M1, C = untangle_cols(LOG2M1), L = M1 * C, PITCH = C + 1, T = UNTANGLE_THREADS;
    extern __shared__ float4 lds[];
    float2* const ta = reinterpret_cast<float2*>(lds);       // [M1][C + 1]: columns a .. a + C - 1
    float2* const tb = ta + M1 * PITCH;                      // [M1][C + 1]: columns M2 - a - C .. M2 - a
    const int log2m = p.log2n - 1, m2 = 1 << (log2m - LOG2M1), m = 1 << log2m;
    const int tid = threadIdx.x;
    const int a = (int)blockIdx.x * C, b0 = m2 - a - C, k0 = a * M1;
    const long base = (long)blockIdx.y << log2m;
    const float2* const z = p.z + base;
    for (int e = tid; e < M1 * C; e += T) {
        const int r = e / C, c = e - r * C;
        ta[r * PITCH + c] = z[(long)r * m2 + a + c];
    }
    for (int e = tid; e < M1 * (C + 1); e += T) {
        const int r = e / (C + 1), c = e - r * (C + 1);
        if (b0 + c < m2) tb[r * PITCH + c] = z[(long)r * m2 + b0 + c];   // column M2 would be bin M + r: only k = 0 mirrors there
    }
    __syncthreads();
    float* const pw = p.pw + base;
    float* const power = p.power ? p.power + ((long)(p.trial0 + (int)blockIdx.y) << log2m) : nullptr;
    for (int i = tid; i < L; i += T) {
        const int k = k0 + i;
        const f2 za = ta[(i & (M1 - 1)) * PITCH + (i >> LOG2M1)];
        float pk;
        if (k == 0) {
            const float dc = za.x + za.y;
            pk = dc * dc;
        } else {
            const int km = m - k;
            const f2 zb = tb[(km & (M1 - 1)) * PITCH + ((km >> LOG2M1) - b0)];
            const stages::Pair x = stages::untangle(za, zb, p.tw[k]);
            pk = stages::power(x.a);
            const float pm = stages::power(x.b);
            pw[km] = pm;
            if (power) __builtin_nontemporal_store(pm, power + km);
        }
        pw[k] = pk;
        if (power) __builtin_nontemporal_store(pk, power + k);
    }
    if (k0 + L == m / 2 && tid == 0) {                       // the bin that is its own mirror: row 0, column M2 / 2
        const int k = m / 2;
        const f2 zh = tb[0];
        const float pk = stages::power(stages::untangle(zh, zh, p.tw[k]).a);
        pw[k] = pk;
        if (power) __builtin_nontemporal_store(pk, power + k);
    }
}

// ---- whiten: workgroup (span, trial); thread i owns bins 16 i .. 16 i + 15 of the span, period.hip's stage 4 ----
__global__ __launch_bounds__(SPAN_THREADS) void whiten_kernel(const Params p)
{
    constexpr int WAVES = SPAN_THREADS / LANES;
    __shared__ float wave_sums[WAVES];
    const int tid = threadIdx.x, lane = tid & (LANES - 1), wave = tid / LANES;
    const int log2m = p.log2n - 1;
    const long off = (long)blockIdx.x * SPAN + 16 * tid;
    float* const pw = p.pw + ((long)blockIdx.y << log2m) + off;
    float v[16];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const float4 f = reinterpret_cast<const float4*>(pw)[q];
        v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
    }
    // the halving tree: adjacent pairs first, one rounding per addition
    float s[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) s[i] = v[2 * i] + v[2 * i + 1];
#pragma unroll
    for (int i = 0; i < 4; ++i) s[i] = s[2 * i] + s[2 * i + 1];
    s[0] = s[0] + s[1];
    s[1] = s[2] + s[3];
    float bsum = s[0] + s[1];
    const int more = p.log2norm - 4;                         // levels behind a thread's 16 bins
    // a + b = b + a bit for bit: the exchange gives both lanes of a pair the pair's sum
#pragma unroll
    for (int lv = 0; lv < 6; ++lv)
        if (lv < more) bsum = bsum + __shfl_xor(bsum, 1 << lv);
    if (more > 6) {                                          // a block of 2 .. 16 wavefronts
        if (lane == 0) wave_sums[wave] = bsum;
        __syncthreads();
        const int g = 1 << (more - 6), first = wave & ~(g - 1);
        float a[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) a[i] = i < g ? wave_sums[first + i] : 0.0f;
#pragma unroll
        for (int w = 2; w <= 16; w <<= 1) {
            if (w <= g) {
#pragma unroll
                for (int i = 0; i < 16 / w; ++i) a[i] = a[2 * i] + a[2 * i + 1];
            }
        }
        bsum = a[0];
    }
    const float bmean = bsum * p.norm_scale;
#pragma unroll
    for (int i = 0; i < 16; ++i) v[i] = v[i] / bmean;        // IEEE division, correctly rounded
#pragma unroll
    for (int q = 0; q < 4; ++q) reinterpret_cast<float4*>(pw)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    if (p.white) {
        float* const dst = p.white + ((long)(p.trial0 + (int)blockIdx.y) << log2m) + off;
#pragma unroll
        for (int q = 0; q < 4; ++q) store_nt<float, 4>(dst + 4 * q, {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]});
    }
}

// ---- peaks: workgroup (span, trial); a wavefront walks a chunk of k, a lane every 64th, period.hip's stage 5 ----
__global__ __launch_bounds__(SPAN_THREADS) void peaks_kernel(const Params p)
{
    constexpr int WAVES = SPAN_THREADS / LANES;
    __shared__ float part_best[MAX_LEVELS * 16];
    __shared__ int part_at[MAX_LEVELS * 16];
    const int tid = threadIdx.x, lane = tid & (LANES - 1), wave = tid / LANES;
    const int log2m = p.log2n - 1;
    const float* const pw = p.pw + ((long)blockIdx.y << log2m);
    const long trial = p.trial0 + (int)blockIdx.y;
    const int levels = p.levels, seg = p.seg, klo = p.klo;
    const int chunk = chunk_of(SPAN, seg), nchunks = SPAN / chunk, nseg = (1 << log2m) / seg;
    const int kb = (int)blockIdx.x * SPAN, segb = kb / seg;  // the span's first bin and segment
    const float ninf = -__builtin_huge_valf();
    for (int c = wave; c < nchunks; c += WAVES) {
        float best[MAX_LEVELS];
        int at[MAX_LEVELS];
#pragma unroll
        for (int l = 0; l < MAX_LEVELS; ++l) best[l] = ninf, at[l] = -1;
        for (int k = kb + c * chunk + lane; k < kb + (c + 1) * chunk; k += LANES) {
            const bool in = k >= klo;
            float acc = pw[k];
            if (in && acc > best[0]) best[0] = acc, at[0] = k;
#pragma unroll
            for (int l = 1; l < MAX_LEVELS; ++l) {
                if (l < levels) {
#pragma unroll
                    for (int h = 1; h < (1 << l); h += 2) acc = acc + pw[((long)k * h + (1 << (l - 1))) >> l];
                    if (in && acc > best[l]) best[l] = acc, at[l] = k;
                }
            }
        }
#pragma unroll
        for (int l = 0; l < MAX_LEVELS; ++l) {
            if (l < levels) {
                meet_lanes(best[l], at[l]);
                if (lane == 0) {
                    if (chunk == seg) {
                        const long o = (trial * levels + l) * nseg + segb + c;
                        p.best[o] = best[l];
                        p.at[o] = at[l];
                    } else {                                 // chunks of 1024: c < 16
                        part_best[l * 16 + c] = best[l];
                        part_at[l * 16 + c] = at[l];
                    }
                }
            }
        }
    }
    if (chunk != seg) {                                      // segments of 2 .. 16 chunks
        __syncthreads();
        const int per = seg / chunk, here = SPAN / seg;
        for (int o = tid; o < levels * here; o += SPAN_THREADS) {
            const int l = o / here, s = o - l * here;
            float best = ninf;
            int at = -1;
            for (int c = s * per; c < (s + 1) * per; ++c) meet(best, at, part_best[l * 16 + c], part_at[l * 16 + c]);
            p.best[(trial * levels + l) * nseg + segb + s] = best;
            p.at[(trial * levels + l) * nseg + segb + s] = at;
        }
    }
}

using Log2M2s = Vals<11, 12, 13, 14>;
using Log2M1s = Vals<4, 8>;

hipError_t launch_head(const Params& p, int group, hipStream_t st)
{
    const int n = p.log2n, l1 = log2m1_of(n);
    const hipError_t e = launch(&mean_kernel, dim3((unsigned)stage_blocks(STAGE_MEAN, n), (unsigned)group), dim3((unsigned)stage_threads(STAGE_MEAN, n)), 0, st, p);
    if (e != hipSuccess) return e;
    return launch(l1 == 4 ? &cols16_kernel : &cols256_kernel, dim3((unsigned)stage_blocks(STAGE_COLS, n), (unsigned)group),
                  dim3((unsigned)stage_threads(STAGE_COLS, n)), (size_t)cols_lds(l1), st, p);
}

hipError_t launch_tail(const Params& p, int group, hipStream_t st)
{
    const int n = p.log2n, l1 = log2m1_of(n), l2 = log2m2_of(n);
    const auto grid = [&](int stage) { return dim3((unsigned)stage_blocks(stage, n), (unsigned)group); };
    const auto block = [&](int stage) { return dim3((unsigned)stage_threads(stage, n)); };
    hipError_t e = pick(Log2M2s{}, l2, [&](auto m) {
        return launch(&rows_kernel<decltype(m)::value>, grid(STAGE_ROWS), block(STAGE_ROWS), (size_t)rows_lds(decltype(m)::value), st, p);
    });
    if (e != hipSuccess) return e;
    e = pick(Log2M1s{}, l1, [&](auto m) {
        return launch(&untangle_kernel<decltype(m)::value>, grid(STAGE_UNTANGLE), block(STAGE_UNTANGLE), (size_t)untangle_lds(decltype(m)::value), st, p);
    });
    if (e != hipSuccess) return e;
    e = launch(&whiten_kernel, grid(STAGE_WHITEN), block(STAGE_WHITEN), 0, st, p);
    if (e != hipSuccess) return e;
    return launch(&peaks_kernel, grid(STAGE_PEAKS), block(STAGE_PEAKS), 0, st, p);
}

hipError_t launch_group(const Params& p, int group, hipStream_t st)
{
    const hipError_t e = launch_head(p, group, st);
    return e != hipSuccess ? e : launch_tail(p, group, st);
}

hipError_t prepare(int log2n, int device)
{
    const int l1 = log2m1_of(log2n), l2 = log2m2_of(log2n);
    hipError_t e = load_kernel(&mean_kernel);
    if (e == hipSuccess) e = load_kernel(&cols16_kernel);
    if (e == hipSuccess) e = load_kernel(&cols256_kernel);
    if (e == hipSuccess) e = load_kernel(&whiten_kernel);
    if (e == hipSuccess) e = load_kernel(&peaks_kernel);
    if (e != hipSuccess) return e;
    e = pick(Log2M2s{}, l2, [&](auto m) {
        const hipError_t g = load_kernel(&rows_kernel<decltype(m)::value>);
        return g != hipSuccess ? g : lds_opt_in(&rows_kernel<decltype(m)::value>, device, (size_t)rows_lds(decltype(m)::value));
    });
    if (e != hipSuccess) return e;
    return pick(Log2M1s{}, l1, [&](auto m) {
        const hipError_t g = load_kernel(&untangle_kernel<decltype(m)::value>);
        return g != hipSuccess ? g : lds_opt_in(&untangle_kernel<decltype(m)::value>, device, (size_t)untangle_lds(decltype(m)::value));
    });
}

}  // namespace periodlong
}  // namespace rtlws

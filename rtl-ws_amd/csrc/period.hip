// period.hip -- the kernel of include/rtlws_period.h (librtlws_period.so): one workgroup takes one trial's
// series from the load to the peaks, the series in LDS all the way.  One instantiation per frame length, and their
// launch table.
//
//   1  load (16-byte loads masked at nsamp), the mean in f64, y = x - mean packed as M complex points into the tile
//   2  the M-point transform in place (row_fft.h)
//   3  the real-input untangling and the square: P[k] over the tile as f32, k < M
//   4  the whitening blocks' halving trees (registers, then lanes, then wavefronts), W = P / mean over P
//   5  the harmonic sums, lanes along k, and the peaks of every level and segment
// meet and meet_lanes are period_stages.h's.  Stages 3, 4 and 5 are written out here; periodlong.hip restates 4 and 5 over
// spans of a row in device memory and takes 3 from period_stages.h (DESIGN.md 4.24a says why the text is not one).
#include <hip/hip_runtime.h>

#include "period.h"
#include "period_stages.h"
#include "row_fft.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace period {

using stages::meet;
using stages::meet_lanes;

template <int LOG2N>
__global__ __launch_bounds__(threads_of(LOG2N)) void period_kernel(const Params p)
{
    constexpr int N = 1 << LOG2N, M = N / 2, T = threads_of(LOG2N), WAVES = T / LANES;
    constexpr int V = N / (4 * T);                           // 16-byte loads per thread
    constexpr int PAIRS = M / (2 * T);                       // bins k and M - k per thread
    extern __shared__ float4 lds[];
    float2* const tile = reinterpret_cast<float2*>(lds);
    float* const pw = reinterpret_cast<float*>(lds);         // P, then W: floats 0 .. M - 1
    float* const wave_sums = pw + M;                         // behind them, free once the tile is read: WAVES floats
    float* const part_best = pw + M + 32;                    // [MAX_LEVELS][16]
    int* const part_at = reinterpret_cast<int*>(pw + M + 32 + MAX_LEVELS * 16);
    static_assert(2 * rowfft::Shape<LOG2N - 1>::TILE_F2 >= M + 32 + 2 * MAX_LEVELS * 16 && WAVES <= 16, "the wavefronts' sums and the partial peaks fit behind W");

    const int tid = threadIdx.x, lane = tid & (LANES - 1), wave = tid / LANES;
    const long trial = blockIdx.x;
    const float* const x = p.in + trial * p.in_stride;
    const int nsamp = p.nsamp;

    // ---- 1: the load and the mean ----
    float4 xv[V];
    double sum = 0.0;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int n0 = 4 * (tid + j * T);
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (n0 + 4 <= nsamp) {
            v = *reinterpret_cast<const float4*>(x + n0);
        } else if (n0 < nsamp) {                             // the last, partial quad: nothing at or behind nsamp is read
            v.x = x[n0];
            if (n0 + 1 < nsamp) v.y = x[n0 + 1];
            if (n0 + 2 < nsamp) v.z = x[n0 + 2];
        }
        xv[j] = v;
        sum += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
    }
#pragma unroll
    for (int off = 1; off < LANES; off <<= 1) sum += __shfl_xor(sum, off);
    double* const dsum = reinterpret_cast<double*>(lds);
    if (lane == 0) dsum[wave] = sum;
    __syncthreads();
    double total = 0.0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) total += dsum[w];
    const double mean = total / (double)nsamp;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const int i = tid + j * T, n0 = 4 * i;
        const float4 v = xv[j];
        float y[4] = {(float)((double)v.x - mean), (float)((double)v.y - mean), (float)((double)v.z - mean), (float)((double)v.w - mean)};
#pragma unroll
        for (int c = 0; c < 4; ++c)
            if (n0 + c >= nsamp) y[c] = 0.0f;
        float2* const z = tile + rowfft::place(2 * i);       // 2 i and 2 i + 1 lie in one group of 16
        z[0] = make_float2(y[0], y[1]);
        z[1] = make_float2(y[2], y[3]);
    }
    __syncthreads();

    // ---- 2: the transform ----
    rowfft::forward<LOG2N - 1>(tile, tid, p.tw);

    // ---- 3: X[k] = E - i W^k O, X[M - k] = conj(E) - i conj(W^k O), E, O = (Z[k] +- conj Z[M - k]) / 2; k = 1 .. M / 2 ----
    {
        f2 za[PAIRS], zb[PAIRS];
#pragma unroll
        for (int j = 0; j < PAIRS; ++j) {
            const int k = 1 + tid + j * T;
            za[j] = tile[rowfft::place(rowfft::pos<LOG2N - 1>(k))];
            zb[j] = tile[rowfft::place(rowfft::pos<LOG2N - 1>(M - k))];
        }
        const f2 z0 = tile[0];
        __syncthreads();                                     // P goes over the tile
#pragma unroll
        for (int j = 0; j < PAIRS; ++j) {
            const int k = 1 + tid + j * T;
            const float2 w = p.tw[k];
            const f2 e = mk(0.5f * (za[j].x + zb[j].x), 0.5f * (za[j].y - zb[j].y));
            const f2 o = mk(0.5f * (za[j].x - zb[j].x), 0.5f * (za[j].y + zb[j].y));
            const f2 t = cmul(o, mk(w.x, w.y));
            const float ax = e.x + t.y, ay = e.y - t.x, bx = e.x - t.y, by = e.y + t.x;
            pw[k] = fmaf(ax, ax, ay * ay);
            if (2 * k != M) pw[M - k] = fmaf(bx, bx, by * by);
        }
        if (tid == 0) {
            const float dc = z0.x + z0.y;
            pw[0] = dc * dc;
        }
    }
    __syncthreads();

    // ---- 4: the whitening: thread i owns bins 16 i .. 16 i + 15 ----
    {
        const bool mine = tid < M / 16;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 f = mine ? reinterpret_cast<const float4*>(pw)[4 * tid + q] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            v[4 * q] = f.x, v[4 * q + 1] = f.y, v[4 * q + 2] = f.z, v[4 * q + 3] = f.w;
        }
        if (p.power && mine) {
            float* const dst = p.power + trial * M + 16 * tid;
#pragma unroll
            for (int q = 0; q < 4; ++q) store_nt<float, 4>(dst + 4 * q, {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]});
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
        const int more = p.log2norm - 4;                     // levels behind a thread's 16 bins
        // a + b = b + a bit for bit: the exchange gives both lanes of a pair the pair's sum
#pragma unroll
        for (int lv = 0; lv < 6; ++lv)
            if (lv < more) bsum = bsum + __shfl_xor(bsum, 1 << lv);
        if (more > 6) {                                      // a block of 2 .. 16 wavefronts
            if (lane == 0) wave_sums[wave] = bsum;
            __syncthreads();
            const int g = 1 << (more - 6), first = wave & ~(g - 1);
            float a[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) a[i] = i < g && first + i < WAVES ? wave_sums[first + i] : 0.0f;
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
        for (int i = 0; i < 16; ++i) v[i] = v[i] / bmean;    // IEEE division, correctly rounded
        if (mine) {
#pragma unroll
            for (int q = 0; q < 4; ++q) reinterpret_cast<float4*>(pw)[4 * tid + q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            if (p.white) {
                float* const dst = p.white + trial * M + 16 * tid;
#pragma unroll
                for (int q = 0; q < 4; ++q) store_nt<float, 4>(dst + 4 * q, {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]});
            }
        }
    }
    __syncthreads();

    // ---- 5: the harmonic sums and the peaks: a wavefront walks a chunk of k, a lane every 64th ----
    {
        const int levels = p.levels, seg = p.seg, klo = p.klo;
        const int chunk = chunk_of(M, seg), nchunks = M / chunk, nseg = M / seg;
        const float ninf = -__builtin_huge_valf();
        for (int c = wave; c < nchunks; c += WAVES) {
            float best[MAX_LEVELS];
            int at[MAX_LEVELS];
#pragma unroll
            for (int l = 0; l < MAX_LEVELS; ++l) best[l] = ninf, at[l] = -1;
            for (int k = c * chunk + lane; k < (c + 1) * chunk; k += LANES) {
                const bool in = k >= klo;
                float acc = pw[k];
                if (in && acc > best[0]) best[0] = acc, at[0] = k;
#pragma unroll
                for (int l = 1; l < MAX_LEVELS; ++l) {
                    if (l < levels) {
#pragma unroll
                        for (int h = 1; h < (1 << l); h += 2) acc = acc + pw[(k * h + (1 << (l - 1))) >> l];
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
                            const long o = (trial * levels + l) * nseg + c;
                            p.best[o] = best[l];
                            p.at[o] = at[l];
                        } else {
                            part_best[l * 16 + c] = best[l];
                            part_at[l * 16 + c] = at[l];
                        }
                    }
                }
            }
        }
        if (chunk != seg) {                                  // segments of 2 .. 16 chunks
            __syncthreads();
            const int per = seg / chunk;
            for (int o = tid; o < levels * nseg; o += T) {
                const int l = o / nseg, s = o - l * nseg;
                float best = ninf;
                int at = -1;
                for (int c = s * per; c < (s + 1) * per; ++c) meet(best, at, part_best[l * 16 + c], part_at[l * 16 + c]);
                p.best[(trial * levels + l) * nseg + s] = best;
                p.at[(trial * levels + l) * nseg + s] = at;
            }
        }
    }
}

using Log2Ns = Vals<10, 11, 12, 13, 14, 15>;
static_assert(MIN_LOG2N == 10 && MAX_LOG2N == 15, "period.h and the launch table disagree");

hipError_t launch_period(int log2n, const Params& p, int ntrials, hipStream_t st)
{
    return pick(Log2Ns{}, log2n, [&](auto n) {
        return launch(&period_kernel<decltype(n)::value>, dim3((unsigned)ntrials), dim3(threads_of(decltype(n)::value)), (size_t)lds_bytes(decltype(n)::value), st, p);
    });
}

hipError_t prepare_period(int log2n, int device)
{
    return pick(Log2Ns{}, log2n, [&](auto n) {
        const hipError_t e = load_kernel(&period_kernel<decltype(n)::value>);
        return e != hipSuccess ? e : lds_opt_in(&period_kernel<decltype(n)::value>, device, (size_t)lds_bytes(decltype(n)::value));
    });
}

}  // namespace period
}  // namespace rtlws

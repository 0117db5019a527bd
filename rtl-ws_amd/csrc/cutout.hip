// cutout.hip -- the kernels of include/rtlws_cutout.h (librtlws_cutout.so): around every candidate of
// the sift's list the waterfall dedispersed at the candidate's trial and summed into time bins and subbands, and the
// series of the neighbouring trials summed into the same bins; two launches.
//
// Both read the list where the sift left it.  The candidate's words, the count, the plan's {w_k, bin_k} and everything
// derived from them (n0, b, the clip of the window) are the same for a whole workgroup and come as scalar loads; the
// workgroups of candidates at or beyond min(d_count[0], max_cand) leave on that scalar before anything else.
// Band-time: lanes run along channels, so the loads of a row are consecutive but for the sweep; a lane walks the rows of
// its channel through the workgroup's bins, DEPTH loads in flight, one f32 addition a row in ascending row, and leaves a
// bin's sum (R of the header) in the tile of LDS.  A row outside the window and a channel the mask leaves out are not
// read; +0.0 stands for them, which an accumulator that began at +0.0 takes without changing a bit (it is never -0.0).
// Behind one barrier thread (f, x) adds the channels of subband f in ascending channel.  Where a subband is wider than
// the tile the workgroup owns one subband and walks it in chunks, thread x carrying the subband's sum from chunk to chunk.
// DM-time: a thread a bin, the b samples of it in ascending n.
// This unit is compiled without contraction; there is nothing but additions in it.
#include <hip/hip_runtime.h>

#include "cutout.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace cutout {

// the list, the count and the plan's tables through the constant address space: loads at a workgroup-uniform index are
// scalar loads
template <typename T>
using Constant = const __attribute__((address_space(4))) T*;
template <typename T>
__device__ __forceinline__ Constant<T> constant(const T* p) { return (Constant<T>)(p); }

// candidate i's window: trial t, rows per bin b, first row n0; valid 0: the header's invalid candidate, t = b = n0 = 0
struct Window {
    int t, b, n0, valid;
};

__device__ __forceinline__ bool served(const Params& p, int i)
{
    const int count = constant(p.count)[0];
    return i < (count < p.max_cand ? count : p.max_cand);
}

__device__ __forceinline__ Window window_of(const Params& p, int i)
{
    const Constant<uint32_t> words = constant(p.cand) + (long)i * CAND_WORDS;          // {t, s, k, at, ..}
    const int t = (int)words[0], k = (int)words[2], at = (int)words[3];
    Window w;
    w.valid = (unsigned)t < (unsigned)p.ntrials && (unsigned)k < (unsigned)p.K && (unsigned)at < (unsigned)p.nsamp;
    const Constant<int> shape = constant(reinterpret_cast<const int*>(p.shape)) + 2 * (w.valid ? k : 0);        // {w_k, bin_k}
    const int width = shape[0], bin = shape[1];
    w.t = w.valid ? t : 0;
    w.b = w.valid ? bin : 0;
    w.n0 = w.valid ? at + width / 2 - (p.nx / 2) * bin : 0;
    return w;
}

__device__ __forceinline__ void write_info(const Params& p, int i, const Window& w)
{
    const int end = w.n0 + p.nx * w.b;
    const int inside = (end < p.nsamp ? end : p.nsamp) - (w.n0 > 0 ? w.n0 : 0);
    int32_t* const info = p.info + (long)i * INFO_WORDS;      // held to 4 bytes, not to 16
    info[0] = w.n0, info[1] = w.b, info[2] = w.valid, info[3] = w.valid && inside > 0 ? inside : 0;
}

template <bool WALK>
__global__ __launch_bounds__(THREADS) void cutout_band_kernel(const Params p)
{
    __shared__ BandLds lds;
    const int tid = threadIdx.x;
    const int fg = (int)(blockIdx.x % (unsigned)p.fgroups), rest = (int)(blockIdx.x / (unsigned)p.fgroups);
    const int xg = rest % p.xgroups, i = rest / p.xgroups;
    if (!served(p, i)) return;                                // the same for the whole workgroup
    const Window w = window_of(p, i);
    if (tid == 0 && xg == 0 && fg == 0) write_info(p, i, w);

    const int nx = p.nx, cpb = p.cpb, b = w.b;
    const int x0 = xg * TILE_X, xb = nx - x0 < TILE_X ? nx - x0 : TILE_X;        // the bins of this workgroup
    const int f0 = fg * p.per, fs = p.nf - f0 < p.per ? p.nf - f0 : p.per;        // its subbands
    float* const out = p.ft + ((long)i * p.nf + f0) * nx + x0;
    if (!w.valid) {
        for (int q = tid; q < fs * TILE_X; q += THREADS)
            if ((q & (TILE_X - 1)) < xb) out[(long)(q / TILE_X) * nx + (q & (TILE_X - 1))] = 0.0f;
        return;
    }

    // rows m = 0 .. total - 1 of the workgroup are n = nbeg + m; those with lo <= m < hi lie inside 0 .. nsamp - 1
    const int nbeg = w.n0 + x0 * b, total = xb * b;
    const int lo = nbeg < 0 ? -nbeg : 0, hi = p.nsamp - nbeg < total ? p.nsamp - nbeg : total;
    const uint16_t* const delays = p.delays + (long)w.t * p.nchan;
    const int chunks = WALK ? (cpb + TILE_C - 1) / TILE_C : 1;
    float carry = 0.0f;                                       // WALK: thread x's sum over the chunks so far
    for (int chunk = 0; chunk < chunks; ++chunk) {
        const int width = WALK ? (cpb - chunk * TILE_C < TILE_C ? cpb - chunk * TILE_C : TILE_C) : fs * cpb;
        const int c = f0 * cpb + chunk * TILE_C + tid;
        const bool keep = tid < width && p.keep[c];
        const int base = nbeg + (keep ? (int)delays[c] : 0);
        float acc = 0.0f;
        int j = 0, x = 0;
        for (int m0 = 0; m0 < total; m0 += DEPTH) {
            float v[DEPTH];
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const int m = m0 + u;
                v[u] = keep && m >= lo && m < hi ? p.rows[(long)(base + m) * p.in_stride + c] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                if (m0 + u >= total) break;
                acc += v[u];
                if (++j == b) {
                    lds.tile[x * TILE_STRIDE + tid] = acc;
                    acc = 0.0f, j = 0, ++x;
                }
            }
        }
        __syncthreads();
        if (WALK) {
            if (tid < xb) {
                const float* const r = lds.tile + tid * TILE_STRIDE;
                for (int cc = 0; cc < width; ++cc) carry += r[cc];
            }
            __syncthreads();                                  // the next chunk stores into the tile
        } else {
            for (int q = tid; q < fs * TILE_X; q += THREADS) {
                const int f = q / TILE_X, xx = q & (TILE_X - 1);
                if (xx >= xb) continue;
                const float* const r = lds.tile + xx * TILE_STRIDE + f * cpb;
                float sum = 0.0f;
                for (int cc = 0; cc < cpb; ++cc) sum += r[cc];
                out[(long)f * nx + xx] = sum;
            }
        }
    }
    if (WALK && tid < xb) out[tid] = carry;
}
static_assert(sizeof(BandLds) <= 64 * 1024 && TILE_X == 32 && TILE_STRIDE % 2 == 1, "static LDS; a half-wavefront's bins on 32 banks");

__global__ __launch_bounds__(THREADS) void cutout_dmt_kernel(const Params p)
{
    const int x = threadIdx.x;
    const int r = (int)(blockIdx.x % (unsigned)p.ndm), i = (int)(blockIdx.x / (unsigned)p.ndm);
    if (!served(p, i)) return;
    const Window w = window_of(p, i);
    if (p.info_from_dmt && r == 0 && x == 0) write_info(p, i, w);
    if (x >= p.nx) return;

    const int q = w.t + (r - p.rq) * p.dq, b = w.b;
    float acc = 0.0f;
    if (w.valid && q >= 0 && q < p.ntrials) {                 // the same for the whole workgroup
        const float* const src = p.series + (long)q * p.series_stride;
        const int n = w.n0 + x * b;
        for (int j0 = 0; j0 < b; j0 += DEPTH) {
            float v[DEPTH];
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) {
                const int nn = n + j0 + u;
                v[u] = j0 + u < b && nn >= 0 && nn < p.nsamp ? src[nn] : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < DEPTH; ++u) acc += v[u];
        }
    }
    p.dmt[((long)i * p.ndm + r) * p.nx + x] = acc;
}

// the launch table: the band-time kernel's two forms and the DM-time kernel; f is handed each in turn until one fails
template <typename F>
static hipError_t with_kernels(F&& f)
{
    hipError_t err = f(&cutout_band_kernel<false>, 0);
    if (err == hipSuccess) err = f(&cutout_band_kernel<true>, 1);
    return err == hipSuccess ? f(&cutout_dmt_kernel, 2) : err;
}

hipError_t launch_cutout(const Params& p, hipStream_t st)
{
    const int band = p.cpb > TILE_C ? 1 : 0;
    return with_kernels([&](auto kernel, int which) {
        if (which == 2) return p.dmt ? launch(kernel, dim3((unsigned)(p.max_cand * p.ndm)), dim3(dmt_threads(p.nx)), 0, st, p) : hipSuccess;
        if (which != band || !p.ft) return hipSuccess;
        return launch(kernel, dim3((unsigned)(p.max_cand * p.xgroups * p.fgroups)), dim3(THREADS), 0, st, p);
    });
}

hipError_t prepare_cutout()
{
    return with_kernels([](auto kernel, int) { return load_kernel(kernel); });
}

}  // namespace cutout
}  // namespace rtlws

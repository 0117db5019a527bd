// pfbbf.hip -- a polyphase beamformer over A = 1 .. 8 coherent cmplx_u8 captures in ONE launch
// (include/rtlws_pfbbf.h): per channel of the filter bank of rtlws_pfb.h, B = 1 .. 4 complex-weighted sums of the
// captures' frames, as voltages or as K-frame powers.
//
//   t_a        = (fl(fl(wr yr) - fl(wi yi)), fl(fl(wr yi) + fl(wi yr)))    w = W[b][a][c], y = Y_a[m][c]: passes 1 .. 4
//   Z_b[m][c]  = (((+0 + t_0) + t_1) + ..) + t_(A-1)                       of the filter bank's tile (pfb_tile.h)
//   P_b[m][c]  = fl(fl(zr zr) + fl(zi zi))
//   S_b[j][c]  = sum_{r < K} P_b[j K + r][c]                               f32, in the spectrometer's order
//
// The beam is linear in the captures, so a workgroup of 256 threads needs ONE tile whatever A and B are: for every
// capture in turn tile_passes<K> fills the tile, every thread reads its 16 items (item tid + 256 i: frame e / M,
// channel e % M, so a thread's channel is one for M <= 256 and M / 256 otherwise), fetches their weights and adds
// w y into its B x 16 complex running values in registers; a barrier, and the tile is refilled.  The order of Z's
// sum is over a alone, so Z does not depend on which thread holds an item.
//   voltage  the channelizer's geometry (pfb_bank.hip): F = 4096 / M frames per workgroup.  Time-major rows are
//            stored from the registers; channel-major goes beam by beam through the tile, free by then, to be read
//            in runs of F frames of a channel.  The sign rule is a sign-bit flip at the store.
//   power    the spectrometer's geometry and order of sums (pfbspec.hip): after the last capture of
//            a tile iteration every beam in turn is written to the tile at place(c) (every thread to the places it
//            read), squared and summed in slices of SLICE = min(16, F) frames from +0.  K >= F: an item is (slice s,
//            bin c), its running slice sum (M / 256 per beam at most 4) stays in a register over the iterations, and
//            the slices are added in the order s = 0, 1, .. through LDS at the end.  K < F: floor(F / K) spectra in
//            the one tile; the thread of (spectrum g, bin c) adds its slices in order itself.  The beams' voltages
//            never reach device memory.
// B is a template parameter 1 .. 4: the running values are B x 32 registers that have to be indexed at compile time
// to stay registers, and an instantiation per B holds exactly what it needs (three workgroups per compute unit at
// B = 1, two at B = 4) where a predicated B = 4 would give every caller the largest.  A is a run-time loop.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_ksum.h"
#include "pfbbf.h"

namespace rtlws {
namespace pfbbf {

using namespace rtlws::pfb;

constexpr int PER = TILE_POINTS / THREADS;            // items of the tile per thread

// w y.  The products pass through an empty asm, as in power() (pfb_ksum.h), so that no sum or difference can take
// one of them into a fused multiply-add
__device__ __forceinline__ float2 weighted(float2 w, float2 y)
{
    float rr = w.x * y.x, ii = w.y * y.y, ri = w.x * y.y, ir = w.y * y.x;
    asm("" : "+v"(rr));
    asm("" : "+v"(ii));
    asm("" : "+v"(ri));
    asm("" : "+v"(ir));
    return make_float2(rr - ii, ri + ir);
}

// item i of thread tid: e = tid + 256 i is frame e / M of the tile, channel e % M
template <int K>
__device__ __forceinline__ int item_place(int tid, int i)
{
    const int e = tid + THREADS * i;
    return (e >> K) * row_stride(K) + place(e & ((1 << K) - 1));
}

// z[b][i] += W[b][a][c] Y_a of the thread's items; w points at W[0][a][0], beam b lies b * wstride further
template <int K, int B>
__device__ __forceinline__ void add_capture(const float2* tile, const float2* w, int wstride, int tid, float2 (&z)[B][PER])
{
    constexpr int M = 1 << K, NC = M > THREADS ? M / THREADS : 1;     // the channels of a thread: tid + 256 j
    float2 wt[B][NC];
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int j = 0; j < NC; ++j) wt[b][j] = w[b * wstride + ((tid + THREADS * j) & (M - 1))];
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const float2 y = tile[item_place<K>(tid, i)];
#pragma unroll
        for (int b = 0; b < B; ++b) {
            const float2 t = weighted(wt[b][i % NC], y);
            z[b][i].x = z[b][i].x + t.x;
            z[b][i].y = z[b][i].y + t.y;
        }
    }
}

// Every capture in turn through the tile; afterwards z holds Z_b of the tile's frames from m0 on, and every thread
// has passed a barrier behind its last read of the tile
template <int K, int B>
__device__ __forceinline__ void beams_of_tile(const BfParams& p, PfbParams& bank, long m0, int tid, float2* tile, float2 (&z)[B][PER])
{
    constexpr int M = 1 << K;
#pragma unroll
    for (int b = 0; b < B; ++b)
#pragma unroll
        for (int i = 0; i < PER; ++i) z[b][i] = make_float2(0.0f, 0.0f);
    const int A = p.ninputs;
#pragma unroll 1
    for (int a = 0; a < A; ++a) {
        bank.src = p.src[a];
        int t = tile_passes_afresh<K>(bank, m0, tid, tile);
        asm volatile("" : "+v"(t));                                      // nor the accumulate step's places and addresses
        add_capture<K, B>(tile, p.w + (long)a * M, A * M, t, z);
        __syncthreads();                                                 // before the tile is refilled
    }
}

template <int K, int B>
__global__ __launch_bounds__(THREADS) void pfbbf_kernel(const BfParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K);
    __shared__ __attribute__((aligned(16))) float2 tile[F * ROW];
    static_assert(sizeof(tile) == lds_bytes(K), "pfbbf.h and the kernel disagree");

    const int tid = threadIdx.x;
    const long m0 = (long)blockIdx.x * F;
    PfbParams bank = p.bank;
    float2 z[B][PER];
    beams_of_tile<K, B>(p, bank, m0, tid, tile, z);

    // the sign rule of the half hop, as a sign-bit flip of both components: (-1)^(c g), g = first + m
    const unsigned odd_frame0 = bank.half_hop ? (unsigned)(bank.first + m0) & 1u : 0u;
#pragma unroll
    for (int i = 0; i < PER; ++i) {
        const int e = tid + THREADS * i, f = e / M, c = e % M;
        if (bank.half_hop && ((odd_frame0 + f) & c & 1)) {
#pragma unroll
            for (int b = 0; b < B; ++b) z[b][i] = make_float2(-z[b][i].x, -z[b][i].y);
        }
    }
    if (bank.layout == LAYOUT_TIME) {
        // runs of M bins of a frame, from the registers
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float2* out = bank.out + b * p.beam_stride;
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int e = tid + THREADS * i, f = e / M, c = e % M;
                const long m = m0 + f;
                if (m < bank.nframes) out[m * bank.out_stride + c] = z[b][i];
            }
        }
    } else {
        // runs of F frames of a channel: beam by beam through the tile (every thread writes the places it read)
#pragma unroll
        for (int b = 0; b < B; ++b) {
            float2* out = bank.out + b * p.beam_stride;
#pragma unroll
            for (int i = 0; i < PER; ++i) tile[item_place<K>(tid, i)] = z[b][i];
            __syncthreads();
#pragma unroll 4
            for (int i = 0; i < PER; ++i) {
                const int e = tid + THREADS * i, f = e % F, c = e / F;
                const long m = m0 + f;
                if (m < bank.nframes) out[(long)c * bank.out_stride + m] = tile[f * ROW + place(c)];
            }
            if (b + 1 < B) __syncthreads();
        }
    }
}

// WHOLE: K >= F, the workgroup owns one spectrum over ceil(K / F) tile iterations; else floor(F / K) spectra in one
// tile.  The host chooses (the spectrometer's kernel branches on it at run time; two instantiations hold what each
// needs: running slice sums over the iterations here, the spectra's places in the tile there)
template <int K, int B, bool WHOLE>
__global__ __launch_bounds__(THREADS) void pfbbf_power_kernel(const BfParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K), SLICE = slice_frames(K);
    __shared__ __attribute__((aligned(16))) float2 tile[F * ROW];
    static_assert(sizeof(tile) == lds_bytes(K), "pfbbf.h and the kernel disagree");
    static_assert(B * THREADS * sizeof(float) <= sizeof(tile), "the partial sums reuse the tile");

    const int tid = threadIdx.x;
    const int k_avg = p.k_avg, shift = p.shift;
    PfbParams bank = p.bank;
    float2 z[B][PER];

    if constexpr (!WHOLE) {
        // several spectra in the one tile: spectrum g begins at frame g K
        const int G = F / k_avg;                      // spectra_per_block
        const long j0 = (long)blockIdx.x * G;
        beams_of_tile<K, B>(p, bank, j0 * k_avg, tid, tile, z);
        const int nsl = (k_avg + SLICE - 1) / SLICE;
        const int nout = G * M;
#pragma unroll
        for (int b = 0; b < B; ++b) {
            // Z_b to the tile, every thread to the places it read: place(c) of row f holds Z_b[m0 + f][c]
            if (b > 0) __syncthreads();                                  // the tile is free
#pragma unroll
            for (int i = 0; i < PER; ++i) tile[item_place<K>(tid, i)] = z[b][i];
            __syncthreads();
            // the thread of (g, c) forms every slice sum from +0 and adds them in order
            for (int o = tid; o < nout; o += THREADS) {
                const int c = o % M, g = o / M;
                const long j = j0 + g;
                if (j >= p.nspectra) break;
                const float2* src = tile + g * k_avg * ROW + place(c);
                float sum = 0.0f;
                for (int s = 0; s < nsl; ++s) {
                    const int nl = min(SLICE, k_avg - s * SLICE);
                    float sl = 0.0f;
                    for (int l = 0; l < nl; ++l) sl = sl + power(src[(s * SLICE + l) * ROW]);
                    sum = s == 0 ? sl : sum + sl;
                }
                const float o1[1] = {sum};
                store_nt(p.rows + (j * B + b) * p.row_stride + ((c + shift) & (M - 1)), o1);
            }
        }
    } else {
        // item w = s M + c, w = tid + 256 i; a thread's items are the same in every iteration
        constexpr int NW = M > THREADS ? M / THREADS : 1;
        const int nit = (k_avg + F - 1) / F;
        const long j0 = blockIdx.x;
        float acc[B][NW];
#pragma unroll
        for (int b = 0; b < B; ++b)
#pragma unroll
            for (int i = 0; i < NW; ++i) acc[b][i] = 0.0f;

        for (int it = 0; it < nit; ++it) {
            beams_of_tile<K, B>(p, bank, j0 * k_avg + (long)it * F, tid, tile, z);
            // the places of the epilogue are formed in every iteration, as the passes' are
            int t = tid;
            asm volatile("" : "+v"(t));
#pragma unroll
            for (int b = 0; b < B; ++b) {
#pragma unroll
                for (int i = 0; i < PER; ++i) tile[item_place<K>(t, i)] = z[b][i];
                __syncthreads();
                // the powers of a slice's frames, in frame order
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const int w = t + THREADS * i, c = w % M, s = w / M;
                    const int nl = min(SLICE, k_avg - (it * F + s * SLICE));
                    const float2* src = tile + s * SLICE * ROW + place(c);
                    for (int l = 0; l < nl; ++l) acc[b][i] = acc[b][i] + power(src[l * ROW]);
                }
                __syncthreads();                                         // the tile is free
            }
        }

        if constexpr (F == SLICE) {
            // one slice: an item is a bin
#pragma unroll
            for (int b = 0; b < B; ++b)
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const float o1[1] = {acc[b][i]};
                    store_nt(p.rows + (j0 * B + b) * p.row_stride + ((tid + THREADS * i + shift) & (M - 1)), o1);
                }
        } else {
            // the slices in order s = 0, 1, .. through LDS: beam b's sum of item w at part[b * 256 + w]
            static_assert(NW == 1 && (F / SLICE) * M == THREADS, "M < 256: one item per thread, 256 / M slices");
            float* part = reinterpret_cast<float*>(tile);
#pragma unroll
            for (int b = 0; b < B; ++b) part[b * THREADS + tid] = acc[b][0];
            __syncthreads();
            if (tid < M) {
#pragma unroll
                for (int b = 0; b < B; ++b) {
                    float t = part[b * THREADS + tid];
#pragma unroll
                    for (int s = 1; s < F / SLICE; ++s) t = t + part[b * THREADS + s * M + tid];
                    const float o1[1] = {t};
                    store_nt(p.rows + (j0 * B + b) * p.row_stride + ((tid + shift) & (M - 1)), o1);
                }
            }
        }
    }
}

// the launch tables: f is handed the plan's instantiation.  The host chooses WHOLE
using Beams = Vals<1, 2, 3, 4>;
static_assert(MIN_BEAMS == 1 && MAX_BEAMS == 4, "pfbbf.h and the launch tables disagree");

template <typename F>
static hipError_t with_kernel(int k, int nbeams, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) { return pick(Beams{}, nbeams, [&](auto b) { return f(&pfbbf_kernel<kk, b>); }); });
}

template <typename F>
static hipError_t with_power_kernel(int k, int nbeams, bool whole, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) {
        return pick(Beams{}, nbeams, [&](auto b) {
            return pick(Bools{}, whole, [&](auto w) { return f(&pfbbf_power_kernel<kk, b, w>); });
        });
    });
}

hipError_t launch_pfbbf(int k, int nbeams, const BfParams& p, hipStream_t st)
{
    const long blocks = (p.bank.nframes + tile_frames(k) - 1) / tile_frames(k);
    return with_kernel(k, nbeams, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t launch_pfbbf_power(int k, int nbeams, const BfParams& p, hipStream_t st)
{
    const int g = spectra_per_block(k, p.k_avg);
    const long blocks = (p.nspectra + g - 1) / g;
    return with_power_kernel(k, nbeams, p.k_avg >= tile_frames(k),
                             [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_pfbbf(int k, int nbeams)
{
    const auto load = [](auto kernel) { return load_kernel(kernel); };
    hipError_t err = with_kernel(k, nbeams, load);
    if (err == hipSuccess) err = with_power_kernel(k, nbeams, true, load);
    if (err == hipSuccess) err = with_power_kernel(k, nbeams, false, load);
    return err;
}

}  // namespace pfbbf
}  // namespace rtlws

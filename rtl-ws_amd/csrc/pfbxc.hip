// pfbxc.hip -- a polyphase cross-correlator over A = 2 .. 4 coherent cmplx_u8 captures in ONE launch
// (include/rtlws_pfbxc.h): per channel of the filter bank of rtlws_pfb.h, the power of every capture and the
// cross-spectrum of every pair, summed over K consecutive frames.  The channelizer's samples never
// reach device memory.
//
//   P_a[m][c]  = fl(fl(ar ar) + fl(ai ai))                               Y_a[m][c] = ar + i ai: passes 1 .. 4 of the
//   X_ab[m][c] = fl(fl(ar br) + fl(ai bi)) + i fl(fl(ai br) - fl(ar bi))   filter bank's tile (pfb_tile.h), a < b
//   S_a[j][c]  = sum_{r < K} P_a[j K + r][c],  V_ab[j][c] = sum_{r < K} X_ab[j K + r][c]      f32, re and im apart
//
// The geometry and the order of every sum are the spectrometer's (pfbspec.hip): a workgroup of 256
// threads owns one spectrum over ceil(K / F) tile iterations where K >= F = 4096 / M, else floor(F / K) spectra in
// one tile; slices of SLICE = min(16, F) frames are summed in frame order from +0, and the slice sums are added in
// the order s = 0, 1, ...  Every input has a tile of its own, filled by tile_passes<K>; place(c) of row f of tile a
// holds Y_a[m0 + f][c].  Then
//   K >= F  an item is (slice s, bin c), items tid, tid + 256, ..: its A + A (A - 1) running sums stay in registers
//           over the iterations; after the last one the slices are added through LDS (the tiles, free by then) and
//           the thread of bin c stores the A + NX values of that bin;
//   K <  F  the tiles are needed until the last product is formed, so nothing is staged: a thread owns (spectrum g,
//           bin c), adds its slices in order itself and stores from registers.
// Consecutive lanes hold consecutive bins in both, for the LDS reads and for the stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_ksum.h"
#include "pfbxc.h"

namespace rtlws {
namespace pfbxc {

using namespace rtlws::pfb;

// a conj(b).  The products pass through an empty asm, as in power() (pfb_ksum.h), so that no sum or difference can
// take one of them into a fused multiply-add
__device__ __forceinline__ float2 cross(float2 a, float2 b)
{
    float rr = a.x * b.x, ii = a.y * b.y, ir = a.y * b.x, ri = a.x * b.y;
    asm("" : "+v"(rr));
    asm("" : "+v"(ii));
    asm("" : "+v"(ir));
    asm("" : "+v"(ri));
    return make_float2(rr + ii, ir - ri);
}

// The sums of one bin: q = 0 .. A - 1 the powers, then (re, im) of the pairs (0,1), (0,2), .., (1,2), ..
template <int A>
struct Sums {
    static constexpr int NQ = A * A;
    float q[NQ];

    __device__ __forceinline__ void zero()
    {
#pragma unroll
        for (int i = 0; i < NQ; ++i) q[i] = 0.0f;
    }

    // one frame: src is place(c) of the frame's row in tile 0, tile a lies a * tile_stride further
    __device__ __forceinline__ void add_frame(const float2* src, int tile_stride)
    {
        float2 y[A];
#pragma unroll
        for (int a = 0; a < A; ++a) y[a] = src[a * tile_stride];
#pragma unroll
        for (int a = 0; a < A; ++a) q[a] = q[a] + power(y[a]);
        int x = A;
#pragma unroll
        for (int a = 0; a < A; ++a)
#pragma unroll
            for (int b = a + 1; b < A; ++b) {
                const float2 t = cross(y[a], y[b]);
                q[x] = q[x] + t.x;
                q[x + 1] = q[x + 1] + t.y;
                x += 2;
            }
    }

    __device__ __forceinline__ void add(const Sums& o)
    {
#pragma unroll
        for (int i = 0; i < NQ; ++i) q[i] = q[i] + o.q[i];
    }

    // bin c of spectrum j, at its place in the A auto rows and the NX cross rows
    __device__ __forceinline__ void store(const XcParams& p, long j, int pos) const
    {
#pragma unroll
        for (int a = 0; a < A; ++a) {
            const float o[1] = {q[a]};
            store_nt(p.autos + (j * A + a) * p.auto_stride + pos, o);
        }
#pragma unroll
        for (int x = 0; x < pairs(A); ++x) {
            const float o[2] = {q[A + 2 * x], q[A + 2 * x + 1]};
            store_nt(reinterpret_cast<float*>(p.cross + (j * pairs(A) + x) * p.cross_stride + pos), o);
        }
    }
};

template <int K, int A>
__global__ __launch_bounds__(THREADS) void pfbxc_kernel(const XcParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K), SLICE = slice_frames(K);
    constexpr int TILE = F * ROW;                     // complex values of a tile
    constexpr int NQ = A * A;
    __shared__ __attribute__((aligned(16))) float2 tiles[A * TILE];
    static_assert(sizeof(tiles) == lds_bytes(K, A), "pfbxc.h and the kernel disagree");
    static_assert(NQ * THREADS * sizeof(float) <= sizeof(tiles), "the partial sums reuse the tiles");

    const int tid = threadIdx.x;
    const int k_avg = p.k_avg, shift = p.shift;
    const bool whole = k_avg >= F;                    // the workgroup owns one spectrum
    const int G = whole ? 1 : F / k_avg;              // spectra_per_block
    const int nit = whole ? (k_avg + F - 1) / F : 1;
    const long j0 = (long)blockIdx.x * G;

    // K >= F: item w = s M + c, w = tid + 256 i; a thread's items are the same in every iteration
    constexpr int NW = M > THREADS ? M / THREADS : 1;
    Sums<A> acc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) acc[i].zero();

    PfbParams bank = p.bank;
    for (int it = 0; it < nit; ++it) {
        // 1 .. 4: the branch filters and the transform of every row, one input after the other, each into its tile.
        // The thread index and the arrays' addresses are made opaque before every call, as tile_passes_afresh
        // (pfb_ksum.h) does: what the passes derive from them is formed there and not held in registers across the
        // loops.  Spelled out here: through that wrapper the A tiles' addresses compile differently
#pragma unroll 1
        for (int a = 0; a < A; ++a) {
            int t = tid;
            bank.src = p.src[a];
            asm volatile("" : "+v"(t), "+s"(bank.src), "+s"(bank.taps), "+s"(bank.tw));
            tile_passes<K>(bank, j0 * k_avg + (long)it * F, t, tiles + a * TILE);
        }

        // the products of a slice's frames, in frame order
        if (whole) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int w = tid + THREADS * i, c = w % M, s = w / M;
                const int nl = min(SLICE, k_avg - (it * F + s * SLICE));
                const float2* src = tiles + s * SLICE * ROW + place(c);
                for (int l = 0; l < nl; ++l) acc[i].add_frame(src + l * ROW, TILE);
            }
            __syncthreads();                                             // the tiles are free
        }
    }

    if (!whole) {
        // several spectra in the one tile (it stands outside the loop, as in pfbspec.hip): spectrum g begins at
        // frame g K; the thread of (g, c) forms every slice sum from +0 and adds them in order
        const int nsl = (k_avg + SLICE - 1) / SLICE;
        const int nout = G * M;
        for (int o = tid; o < nout; o += THREADS) {
            const int c = o % M, g = o / M;
            const long j = j0 + g;
            if (j >= p.nspectra) break;
            const float2* src = tiles + g * k_avg * ROW + place(c);
            Sums<A> sum;
            for (int s = 0; s < nsl; ++s) {
                const int nl = min(SLICE, k_avg - s * SLICE);
                Sums<A> sl;
                sl.zero();
                for (int l = 0; l < nl; ++l) sl.add_frame(src + (s * SLICE + l) * ROW, TILE);
                if (s == 0) sum = sl;
                else sum.add(sl);
            }
            sum.store(p, j, (c + shift) & (M - 1));
        }
    } else if constexpr (F == SLICE) {
        // one slice: an item is a bin
#pragma unroll
        for (int i = 0; i < NW; ++i) acc[i].store(p, j0, (tid + THREADS * i + shift) & (M - 1));
    } else {
        // the slices in order s = 0, 1, .. through LDS: sum q of item w at part[q * 256 + w]
        static_assert(NW == 1 && (F / SLICE) * M == THREADS, "M < 256: one item per thread, 256 / M slices");
        float* part = reinterpret_cast<float*>(tiles);
#pragma unroll
        for (int q = 0; q < NQ; ++q) part[q * THREADS + tid] = acc[0].q[q];
        __syncthreads();
        if (tid < M) {
            Sums<A> sum;
#pragma unroll
            for (int q = 0; q < NQ; ++q) {
                float t = part[q * THREADS + tid];
#pragma unroll
                for (int s = 1; s < F / SLICE; ++s) t = t + part[q * THREADS + s * M + tid];
                sum.q[q] = t;
            }
            sum.store(p, j0, (tid + shift) & (M - 1));
        }
    }
}

// the launch table: f is handed the plan's instantiation
using Inputs = Vals<2, 3, 4>;
static_assert(MIN_INPUTS == 2 && MAX_INPUTS == 4, "pfbxc.h and the launch table disagree");

template <typename F>
static hipError_t with_kernel(int k, int ninputs, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) { return pick(Inputs{}, ninputs, [&](auto a) { return f(&pfbxc_kernel<kk, a>); }); });
}

hipError_t launch_pfbxc(int k, int ninputs, const XcParams& p, hipStream_t st)
{
    const int g = spectra_per_block(k, p.k_avg);
    const long blocks = (p.nspectra + g - 1) / g;
    return with_kernel(k, ninputs, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_pfbxc(int k, int ninputs)
{
    return with_kernel(k, ninputs, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace pfbxc
}  // namespace rtlws

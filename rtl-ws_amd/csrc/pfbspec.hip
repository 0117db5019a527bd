// pfbspec.hip -- a polyphase spectrometer over a cmplx_u8 capture in ONE launch (include/rtlws_pfbspec.h): the power
// of all M = 2^k channels of the filter bank of rtlws_pfb.h, summed over K consecutive frames, as f32 sums, dB or
// payload bytes.  The channelizer's samples never reach device memory.
//
//   P[m][c] = fl(fl(re re) + fl(im im))       Y[m][c] = re + i im: passes 1 .. 4 of the filter bank's tile (pfb_tile.h)
//   S[j][c] = sum_{r < K} P[j K + r][c]       f32, in an order that (M, K) alone decide
//
// A workgroup of 256 threads owns whole spectra (pfb_bank.h): one spectrum over ceil(K / F) tile iterations where
// K >= F = 4096 / M, else floor(F / K) spectra in one tile.  After pass 4 a row of the tile holds a frame's M bins in
// natural order, and
//   5 square   an item is (spectrum g of the workgroup, slice s, bin c), items tid, tid + 256, ..: consecutive lanes
//              read consecutive bins of a row.  An item adds the powers of its slice's frames, in frame order, into a
//              running sum in a register; over the tile iterations slice s takes the frames it F + s SLICE + l;
//   6 combine  the slices of a spectrum are added in the order s = 0, 1, .. through LDS (the tile, which is free by
//              then), and the finished rows are laid out in LDS in the order of the output (shifted or not);
//   7 store    rows as 16-byte vectors: four f32 sums or dB values, or sixteen payload bytes.
// power() and the passes' call are pfb_ksum.h's; pfbxc.hip and pfbbf.hip restate steps 5 and 6 in this order.
// So S[j][c] = ((A_0 + A_1) + ..) + A_(n-1) with A_s = ((P[s SLICE] + P[s SLICE + 1]) + ..), frames at or behind K
// left out: the order does not know j, the place of a spectrum in its tile or in the grid, T, the hop or the output
// kind (an empty slice would add +0 to a sum that is never negative, which changes no bit).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_ksum.h"
#include "pfbspec.h"

namespace rtlws {
namespace pfbspec {

using namespace rtlws::pfb;

static_assert(OUT_SUM == rtlws::OUT_SUM && OUT_DB == rtlws::OUT_DB && OUT_PAYLOAD == rtlws::OUT_PAYLOAD,
              "pfbspec.h and rtlws_internal.h disagree");

template <int K>
__global__ __launch_bounds__(THREADS) void pfbspec_kernel(const SpecParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K), SLICE = slice_frames(K);
    constexpr int PER = TILE_POINTS / THREADS;        // items per thread at most: K = 1, every point a row value
    __shared__ __attribute__((aligned(16))) float2 tile[F * ROW];
    static_assert(sizeof(tile) == lds_bytes(K), "pfbspec.h and the kernel disagree");
    static_assert(2 * TILE_POINTS * sizeof(float) <= sizeof(tile), "the partial sums and the rows reuse the tile");

    const int tid = threadIdx.x;
    const int k_avg = p.k_avg, shift = p.shift;
    const bool whole = k_avg >= F;                    // the workgroup owns one spectrum
    const int G = whole ? 1 : F / k_avg;              // spectra_per_block
    const int nit = whole ? (k_avg + F - 1) / F : 1;
    const int nsl = whole ? F / SLICE : (k_avg + SLICE - 1) / SLICE;
    const int items = G * nsl * M;                    // <= TILE_POINTS
    const long j0 = (long)blockIdx.x * G;
    float* part = reinterpret_cast<float*>(tile);     // item w's sum at part[w], where a spectrum has several slices
    float* rows = part + TILE_POINTS;                 // the finished rows, in the order of the output

    // item w = (g nsl + s) M + c.  One spectrum: g = 0, a thread's items are the same in every iteration
    constexpr int NW = M > THREADS ? M / THREADS : 1;
    float acc[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) acc[i] = 0.0f;

    PfbParams bank = p.bank;
    for (int it = 0; it < nit; ++it) {
        // 1 .. 4: the branch filters and the transform of every row (pfb_tile.h), their addresses formed afresh
        tile_passes_afresh<K>(bank, j0 * k_avg + (long)it * F, tid, tile);

        // 5: the powers of a slice's frames, in frame order
        if (whole) {
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                const int w = tid + THREADS * i, c = w % M, s = w / M;
                const int nl = min(SLICE, k_avg - (it * F + s * SLICE));
                const float2* src = tile + s * SLICE * ROW + place(c);
                for (int l = 0; l < nl; ++l) acc[i] = acc[i] + power(src[l * ROW]);
            }
            __syncthreads();                                             // the tile is free
        }
    }
    if (!whole) {
        // several spectra in the one tile (it stands outside the loop, which then holds nothing of it in registers):
        // spectrum g begins at frame g K.  gs / nsl by a multiplication, exact for gs < 256 and nsl <= 16
        const int inv = 65536 / nsl + 1;
        float a[PER];
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int w = tid + THREADS * i;
            a[i] = 0.0f;
            if (w < items) {
                const int c = w % M, gs = w / M, g = (gs * inv) >> 16, s = gs - g * nsl;
                const int nl = min(SLICE, k_avg - s * SLICE);
                const float2* src = tile + (g * k_avg + s * SLICE) * ROW + place(c);
                for (int l = 0; l < nl; ++l) a[i] = a[i] + power(src[l * ROW]);
            }
        }
        __syncthreads();                                                 // the tile is free
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int w = tid + THREADS * i;
            if (w < items) {
                if (nsl == 1) rows[(w & ~(M - 1)) | ((w + shift) & (M - 1))] = a[i];
                else part[w] = a[i];
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int w = tid + THREADS * i;
            if (F == SLICE) rows[(w + shift) & (M - 1)] = acc[i];
            else part[w] = acc[i];
        }
    }

    // 6: the slices in order, every sum to its place in the row
    const int nout = G * M;
    if (nsl > 1) {
        __syncthreads();
        for (int o = tid; o < nout; o += THREADS) {
            const int c = o % M, g = o / M;
            const float* q = part + g * nsl * M + c;
            float t = q[0];
            for (int s = 1; s < nsl; ++s) t = t + q[s * M];
            rows[g * M + ((c + shift) & (M - 1))] = t;
        }
    }
    __syncthreads();

    // 7: the rows
    if (p.output == OUT_PAYLOAD) {
        uint8_t* out = static_cast<uint8_t*>(p.out);
        for (int v = tid; v < nout / 16; v += THREADS) {
            const int e = 16 * v;
            const long j = j0 + e / M;
            if (j < p.nspectra) {
                unsigned b[4];
#pragma unroll
                for (int h = 0; h < 4; ++h) {
                    const float4 x = *reinterpret_cast<const float4*>(rows + e + 4 * h);
                    b[h] = payload_byte(payload_db_f32(x.x, p.lin)) | payload_byte(payload_db_f32(x.y, p.lin)) << 8 |
                           payload_byte(payload_db_f32(x.z, p.lin)) << 16 | payload_byte(payload_db_f32(x.w, p.lin)) << 24;
                }
                store_nt(reinterpret_cast<unsigned*>(out + j * p.out_stride + e % M), b);
            }
        }
    } else {
        float* out = static_cast<float*>(p.out);
        for (int v = tid; v < nout / 4; v += THREADS) {
            const int e = 4 * v;
            const long j = j0 + e / M;
            if (j < p.nspectra) {
                const float4 x = *reinterpret_cast<const float4*>(rows + e);
                float o[4] = {x.x, x.y, x.z, x.w};
                if (p.output == OUT_DB) {
#pragma unroll
                    for (int h = 0; h < 4; ++h) o[h] = payload_db_f32(o[h], p.lin);
                }
                store_nt(out + j * p.out_stride + e % M, o);
            }
        }
    }
}

// the launch table: f is handed the plan's instantiation
template <typename F>
static hipError_t with_kernel(int k, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) { return f(&pfbspec_kernel<kk>); });
}

hipError_t launch_pfbspec(int k, const SpecParams& p, hipStream_t st)
{
    const int g = spectra_per_block(k, p.k_avg);
    const long blocks = (p.nspectra + g - 1) / g;
    return with_kernel(k, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_pfbspec(int k)
{
    return with_kernel(k, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace pfbspec
}  // namespace rtlws

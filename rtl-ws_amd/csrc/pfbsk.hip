// pfbsk.hip -- a polyphase spectrometer with spectral-kurtosis excision over a cmplx_u8 capture in ONE launch
// (include/rtlws_pfbsk.h): the power of all M = 2^k channels of the filter bank of rtlws_pfb.h, summed
// over the kept ones of L sub-integrations of K frames each.  Neither the channelizer's samples nor the short rows reach
// device memory unless the caller asks for the latter.
//
//   P        = fl(fl(re re) + fl(im im))        pfb_ksum.h's power(), Y[m][c] = re + i im
//   S1[q][c] = sum P,  S2[q][c] = sum fl(p p)   p = fl(P power_scale); frames q K .. q K + K - 1, pfbspec.hip's order
//   flagged  = fl(K S2) < fl(ratio_lo u) or fl(K S2) > fl(ratio_hi u)      u = fl(s s), s = fl(S1 power_scale)
//   C[j][c]  = ((+0 + S1[j L + l0][c]) + S1[j L + l1][c]) + ..  over the kept l, ascending;  N[j][c] their number
//
// A workgroup of 256 threads owns one output row and walks its L sub-integrations in order.  A sub-integration lies on
// the tile as a spectrum of pfbspec.hip does (pfb_bank.h): over ceil(K / F) tile iterations where K >= F = 4096 / M,
// else floor(F / K) sub-integrations in one tile.  After pass 4 of a tile
//   5 square   pfbspec.hip's items (sub-integration g of the tile, slice s, bin c), two running sums in registers
//              where it has one: the powers and their scaled squares, frame by frame;
//   6 fold     both sets of slice sums go to LDS (the tile, which is free by then: 2 x 4096 floats); the thread that
//              owns bin c (c = tid, tid + 256, ..) adds the slices of S1 and of S2 in the order s = 0, 1, .., decides,
//              adds a kept S1 into its running C and counts it, sub-integration after sub-integration, and stores
//              the S1 and S2 rows where they are asked for;
// and after the last one
//   7 store    C and N through LDS into the order of the output, rows as 16-byte vectors: four f32 sums or dB
//              values, sixteen payload bytes, four uint32 counts.
// So S1[q] is rtlws_pfbspec_run's row q at the same K bit for bit, and no sum knows j, the place of a
// sub-integration in its tile, T, the hop or the output kind.  Every product that an addition follows passes through
// an empty asm, as in power(): the file is compiled with contraction on.  The path (K >= F or not) is a template
// parameter that the host chooses, as in pfbbf.hip: fourteen kernels.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_ksum.h"
#include "pfbsk.h"

namespace rtlws {
namespace pfbsk {

using namespace rtlws::pfb;

static_assert(OUT_SUM == rtlws::OUT_SUM && OUT_DB == rtlws::OUT_DB && OUT_PAYLOAD == rtlws::OUT_PAYLOAD,
              "pfbsk.h and rtlws_internal.h disagree");

// fl(a b), kept out of any fused multiply-add
__device__ __forceinline__ float product(float a, float b)
{
    float r = a * b;
    asm("" : "+v"(r));
    return r;
}

// one frame's bin into the two running sums
__device__ __forceinline__ void square(float2 y, float power_scale, float& a1, float& a2)
{
    const float pw = power(y), ps = product(pw, power_scale);
    a1 = a1 + pw;
    a2 = a2 + product(ps, ps);
}

// the dB value of a clean sum over n kept sub-integrations of kf frames; none kept: -inf, not scale / 0
__device__ __forceinline__ float clean_db(float c, unsigned n, float scale, float kf)
{
    return n ? payload_db_f32(c, scale / product(kf, (float)n)) : -__builtin_inff();
}

// The kernel's arguments behind an address made opaque.  What only the fold or the row's store needs is read through it
// where it is needed: taken at the head of the kernel, as the compiler takes every argument, such values stay in
// scalar registers across the passes, which then spill.  SkParams is the kernel's one parameter, so it lies at the head
// of the argument segment
typedef const __attribute__((address_space(4))) SkParams* Args;
__device__ __forceinline__ Args arguments()
{
    Args a = (Args)__builtin_amdgcn_kernarg_segment_ptr();
    asm volatile("" : "+s"(a));
    return a;
}

// tile_passes_afresh, and its thread index made opaque once more behind the passes' closing barrier: what the items
// derive from it is then formed behind the passes and not among them, where it is held beside pass 4's sixteen points
// (150 VGPRs at M = 256, K < F)
template <int K>
__device__ __forceinline__ int passes_then_items(PfbParams& bank, long m0, int tid, float2* tile)
{
    int t = tile_passes_afresh<K>(bank, m0, tid, tile);
    asm volatile("" : "+v"(t));
    return t;
}

// WHOLE: K >= F, chosen by the host: with both paths in one kernel the scalar registers spill (as in pfbbf.hip)
template <int K, bool WHOLE>
__global__ __launch_bounds__(THREADS) void pfbsk_kernel(const SkParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K), SLICE = slice_frames(K);
    constexpr int PER = TILE_POINTS / THREADS;        // items per thread at most: K = 1, every point a sum
    constexpr int NW = M > THREADS ? M / THREADS : 1; // bins a thread owns; its items where K >= F
    __shared__ __attribute__((aligned(16))) float2 tile[F * ROW];
    static_assert(sizeof(tile) == lds_bytes(K), "pfbsk.h and the kernel disagree");
    static_assert(2 * TILE_POINTS * sizeof(float) <= sizeof(tile), "both sets of slice sums reuse the tile");

    const int tid = threadIdx.x;
    const int k_avg = p.k_avg, nsub = p.nsub, shift = p.shift;
    const float power_scale = p.power_scale, kf = (float)k_avg;
    const int G = WHOLE ? 1 : F / k_avg;              // sub-integrations in a tile
    const int nsl = WHOLE ? F / SLICE : (k_avg + SLICE - 1) / SLICE;
    const long j = blockIdx.x, q0 = j * nsub;         // the row, its first sub-integration
    float* part1 = reinterpret_cast<float*>(tile);    // item w's sums at part1[w] and part2[w]
    float* part2 = part1 + TILE_POINTS;

    float clean[NW];
    unsigned kept[NW];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        clean[i] = 0.0f;
        kept[i] = 0;
    }

    PfbParams bank = p.bank;
    for (int l0 = 0; l0 < nsub; l0 += G) {
        const int gn = min(G, nsub - l0);             // sub-integrations l0 .. l0 + gn - 1 in this step
        // 1 .. 5: item w = (g nsl + s) M + c, as in pfbspec.hip; the thread index comes back opaque from the passes, so
        // what the items and the owners of the bins derive from it is formed after them and not held across them
        int t = tid;
        if constexpr (WHOLE) {
            const int nit = (k_avg + F - 1) / F;
            float a1[NW], a2[NW];
#pragma unroll
            for (int i = 0; i < NW; ++i) a1[i] = a2[i] = 0.0f;
            for (int it = 0; it < nit; ++it) {
                t = passes_then_items<K>(bank, (q0 + l0) * k_avg + (long)it * F, tid, tile);
#pragma unroll
                for (int i = 0; i < NW; ++i) {
                    const int w = t + THREADS * i, c = w % M, s = w / M;
                    const int nl = min(SLICE, k_avg - (it * F + s * SLICE));
                    const float2* src = tile + s * SLICE * ROW + place(c);
                    for (int l = 0; l < nl; ++l) square(src[l * ROW], power_scale, a1[i], a2[i]);
                }
                __syncthreads();                                         // the tile is free
            }
#pragma unroll
            for (int i = 0; i < NW; ++i) {
                part1[t + THREADS * i] = a1[i];
                part2[t + THREADS * i] = a2[i];
            }
        } else {
            // sub-integration g of the tile begins at its frame g K.  gs / nsl by a multiplication, exact for
            // gs < 256 and nsl <= 16.  An item behind the step's last sub-integration adds no frame and stores +0
            t = passes_then_items<K>(bank, (q0 + l0) * k_avg, tid, tile);
            const int inv = 65536 / nsl + 1, items = gn * nsl * M;       // <= TILE_POINTS
            float a1[PER], a2[PER];
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int w = t + THREADS * i;
                const int c = w % M, gs = w / M, g = (gs * inv) >> 16, s = gs - g * nsl;
                const int nl = w < items ? min(SLICE, k_avg - s * SLICE) : 0;
                const float2* src = tile + (g * k_avg + s * SLICE) * ROW + place(c);
                a1[i] = a2[i] = 0.0f;
                for (int l = 0; l < nl; ++l) square(src[l * ROW], power_scale, a1[i], a2[i]);
            }
            __syncthreads();                                             // the tile is free
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                part1[t + THREADS * i] = a1[i];
                part2[t + THREADS * i] = a2[i];
            }
        }
        __syncthreads();

        // 6: the slices in order, the decision, the kept sum
        const Args fold = arguments();
        const float ratio_lo = fold->ratio_lo, ratio_hi = fold->ratio_hi;
        const long sub_stride = fold->sub_stride;
        float *const d_s1 = fold->s1, *const d_s2 = fold->s2;
#pragma unroll
        for (int i = 0; i < NW; ++i) {
            const int c = t + THREADS * i;
            if (c < M) {
                for (int g = 0; g < gn; ++g) {
                    const int w = g * nsl * M + c;
                    float s1 = part1[w], s2 = part2[w];
                    for (int s = 1; s < nsl; ++s) {
                        s1 = s1 + part1[w + s * M];
                        s2 = s2 + part2[w + s * M];
                    }
                    const float sc = product(s1, power_scale), u = product(sc, sc), v = product(kf, s2);
                    const bool flagged = v < product(ratio_lo, u) || v > product(ratio_hi, u);   // false on NaN
                    if (!flagged) {
                        clean[i] = clean[i] + s1;
                        ++kept[i];
                    }
                    if (d_s1) {
                        const long at = (q0 + l0 + g) * sub_stride + ((c + shift) & (M - 1));
                        d_s1[at] = s1;
                        d_s2[at] = s2;
                    }
                }
            }
        }
        __syncthreads();                                                 // the sums are read: the tile may be written
    }

    // 7: the row and its counts in the order of the output
    const Args row = arguments();
    const float scale = row->scale;
    const int output = row->output;
    const long clean_stride = row->clean_stride, kept_stride = row->kept_stride;
    void* const d_clean = row->clean;
    uint32_t* const d_kept = row->kept;
    float* crow = part1;
    unsigned* nrow = reinterpret_cast<unsigned*>(part1 + M);
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const int c = tid + THREADS * i;
        if (c < M) {
            crow[(c + shift) & (M - 1)] = clean[i];
            nrow[(c + shift) & (M - 1)] = kept[i];
        }
    }
    __syncthreads();
    if (output == OUT_PAYLOAD) {
        uint8_t* out = static_cast<uint8_t*>(d_clean);
        for (int v = tid; v < M / 16; v += THREADS) {
            unsigned b[4];
#pragma unroll
            for (int h = 0; h < 4; ++h) {
                const float4 x = *reinterpret_cast<const float4*>(crow + 16 * v + 4 * h);
                const uint4 n = *reinterpret_cast<const uint4*>(nrow + 16 * v + 4 * h);
                b[h] = payload_byte(clean_db(x.x, n.x, scale, kf)) | payload_byte(clean_db(x.y, n.y, scale, kf)) << 8 |
                       payload_byte(clean_db(x.z, n.z, scale, kf)) << 16 | payload_byte(clean_db(x.w, n.w, scale, kf)) << 24;
            }
            store_nt(reinterpret_cast<unsigned*>(out + j * clean_stride + 16 * v), b);
        }
    } else {
        float* out = static_cast<float*>(d_clean);
        for (int v = tid; v < M / 4; v += THREADS) {
            const float4 x = *reinterpret_cast<const float4*>(crow + 4 * v);
            float o[4] = {x.x, x.y, x.z, x.w};
            if (output == OUT_DB) {
                const uint4 n = *reinterpret_cast<const uint4*>(nrow + 4 * v);
                const unsigned nn[4] = {n.x, n.y, n.z, n.w};
#pragma unroll
                for (int h = 0; h < 4; ++h) o[h] = clean_db(o[h], nn[h], scale, kf);
            }
            store_nt(out + j * clean_stride + 4 * v, o);
        }
    }
    if (d_kept) {
        for (int v = tid; v < M / 4; v += THREADS) {
            const uint4 n = *reinterpret_cast<const uint4*>(nrow + 4 * v);
            const unsigned o[4] = {n.x, n.y, n.z, n.w};
            store_nt(d_kept + j * kept_stride + 4 * v, o);
        }
    }
}

// the launch table: f is handed the instantiation of the plan's log2 M and of the run's path
template <typename F>
static hipError_t with_kernel(int k, bool whole, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) { return pick(Bools{}, whole, [&](auto w) { return f(&pfbsk_kernel<kk, w>); }); });
}

hipError_t launch_pfbsk(int k, const SkParams& p, hipStream_t st)
{
    const long blocks = (p.nspectra + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK;
    return with_kernel(k, p.k_avg >= tile_frames(k), [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_pfbsk(int k)
{
    hipError_t err = with_kernel(k, false, [](auto kernel) { return load_kernel(kernel); });
    return err != hipSuccess ? err : with_kernel(k, true, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace pfbsk
}  // namespace rtlws

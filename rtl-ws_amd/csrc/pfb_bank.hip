// pfb_bank.hip -- a polyphase filter bank over a cmplx_u8 capture in ONE launch (include/rtlws_pfb.h): all M = 2^k
// channels of every frame, the prototype's T taps per branch applied in integers, one M-point f32 transform per
// frame.
//
//   v_m[p]  = sum_{t<T} h[p + t M] (x[m D + t M + p] - 128 (1 + i))            int32, exact
//   Y[m][c] = (-1)^(c g) [D = M/2]  sum_p float(v_m[p]) exp(-2 pi i c p / M)    g = first + m
//
// A workgroup of 256 threads owns a tile of F = 4096 / M consecutive frames, 16 points per thread in every phase:
//   1 FIR      a thread owns four adjacent branches p .. p + 3 (one 8-byte load of the capture, one of the taps) of
//              four consecutive frames, whose rows of the capture slide through a window of registers: a row is
//              loaded once for the four frames; 32 int32 accumulators, converted once to f32 into the tile in LDS
//              (one row per frame);
//   2 radix 16 at stride M / 16 over every row, in place, times W_M^(n2 k1);
//   3 radix 16 inside the blocks of M / 16 (M >= 256), in place, times W_(M/16)^(n3 k2);
//   4 radix R  = 2, 4 or 8 over what is left (M = 32, 64, 128, 512, 1024), and every value to its natural bin in
//              the row;
//   5 store    the tile in the order of the layout: runs of M bins of a frame (time-major) or of F frames of a
//              channel (channel-major), the sign rule applied as a sign-bit flip.
// Phases 1 .. 4 are pfb_tile.h's text, which librtlws_pfbspec.so compiles too.
// A frame's values do not depend on its place in a tile or on the other frames: every row goes through the same
// operations in the same order.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pfb_bank.h"
#include "pfb_tile.h"

namespace rtlws {
namespace pfb {

template <int K>
__global__ __launch_bounds__(THREADS) void pfb_kernel(const PfbParams p)
{
    constexpr int M = 1 << K, F = tile_frames(K), ROW = row_stride(K);
    __shared__ float2 tile[F * ROW];
    static_assert(sizeof(tile) == lds_bytes(K), "pfb_bank.h and the kernel disagree");

    const int tid = threadIdx.x;
    const long m0 = (long)blockIdx.x * F;

    // 1 .. 4: the branch filters and the transform of every row (pfb_tile.h)
    tile_passes<K>(p, m0, tid, tile);

    // 5: the stores
    const unsigned odd_frame0 = p.half_hop ? (unsigned)(p.first + m0) & 1u : 0u;
    if (p.layout == LAYOUT_TIME) {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int e = tid + THREADS * i, f = e / M, c = e % M;
            const long m = m0 + f;
            if (m < p.nframes) {
                float2 y = tile[f * ROW + place(c)];
                if (p.half_hop && ((odd_frame0 + f) & c & 1)) y = make_float2(-y.x, -y.y);
                p.out[m * p.out_stride + c] = y;
            }
        }
    } else {
#pragma unroll 4
        for (int i = 0; i < 16; ++i) {
            const int e = tid + THREADS * i, f = e % F, c = e / F;
            const long m = m0 + f;
            if (m < p.nframes) {
                float2 y = tile[f * ROW + place(c)];
                if (p.half_hop && ((odd_frame0 + f) & c & 1)) y = make_float2(-y.x, -y.y);
                p.out[(long)c * p.out_stride + m] = y;
            }
        }
    }
}

// the launch table: f is handed the plan's instantiation
template <typename F>
static hipError_t with_kernel(int k, F&& f)
{
    return pick(Log2Ms{}, k, [&](auto kk) { return f(&pfb_kernel<kk>); });
}

hipError_t launch_pfb(int k, const PfbParams& p, hipStream_t st)
{
    const long blocks = (p.nframes + tile_frames(k) - 1) / tile_frames(k);
    return with_kernel(k, [&](auto kernel) { return launch(kernel, dim3((unsigned)blocks), dim3(THREADS), 0, st, p); });
}

hipError_t prepare_pfb(int k)
{
    return with_kernel(k, [](auto kernel) { return load_kernel(kernel); });
}

}  // namespace pfb
}  // namespace rtlws

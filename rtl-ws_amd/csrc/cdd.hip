// cdd.hip -- the kernel of include/rtlws_cdd.h (librtlws_cdd.so): coherent dedispersion by overlap-save,
// one workgroup per (segment, channel), the segment of N = 2^9 .. 2^14 complex points in one LDS tile from its loads to
// its stores:
//
//   load      8-byte loads of the channel's points s hop .. s hop + N - 1 into place(i)
//   forward   row_fft.h's transform: bin k at place(pos(k))
//   multiply  by the channel's table, which the plan keeps in the order of the places: linear 8-byte reads
//   inverse   row_fft.h's conjugate transpose of forward: point n at place(n), not yet scaled
//   epilogue  points lead .. lead + hop - 1 times 1 / N (a power of two: exact), as voltages or as sums of ksum powers
//
// One kernel text per N serves the voltages and both layouts of the power rows, the choice a uniform branch behind the
// inverse: everything in front of the epilogue is the same instructions whatever is written, so that the power rows are
// the voltages' bits squared and summed (rtlws_cdd.h's promise) by construction; pfb_ksum.h's power keeps the two
// products out of a fused multiply-add.
#include <hip/hip_runtime.h>

#include "cdd.h"
#include "pfb_ksum.h"
#include "row_fft.h"
#include "rtlws_internal.h"

namespace rtlws {
namespace cdd {

template <int LOG2N>
__global__ __launch_bounds__(threads_of(LOG2N)) void cdd_kernel(const Params p)
{
    constexpr int N = 1 << LOG2N, T = threads_of(LOG2N);
    extern __shared__ float4 lds[];
    float2* const tile = reinterpret_cast<float2*>(lds);
    const int tid = threadIdx.x;
    const long seg = blockIdx.x, chan = blockIdx.y;
    const int hop = p.hop, lead = p.lead;

    const float2* const src = p.in + chan * p.in_stride + seg * hop;
#pragma unroll 4
    for (int i = tid; i < N; i += T) tile[rowfft::place(i)] = src[i];
    __syncthreads();
    rowfft::forward<LOG2N>(tile, tid, p.tw);
    const float2* const h = p.table + chan * N;
#pragma unroll 4
    for (int i = tid; i < N; i += T) {
        float2* const at = tile + rowfft::place(i);
        *at = cmul(*at, h[i]);
    }
    __syncthreads();
    // the inverse's passes read the roots forward's passes read, at the same indices: behind an opaque thread index
    // (as pfb_ksum.h's tile_passes_afresh) they are formed and loaded again (the table is in the caches) and not held
    // in registers, or spilled, across the whole transform
    int t = tid;
    asm volatile("" : "+v"(t));
    rowfft::inverse<LOG2N>(tile, t, p.tw);

    const float scale = p.scale;
    const int ksum = p.ksum;
    if (ksum == 0) {
        float2* const dst = reinterpret_cast<float2*>(p.out) + chan * p.out_stride + seg * hop;
        for (int j = tid; j < hop; j += T) {
            const float2 y = tile[rowfft::place(lead + j)];
            dst[j] = make_float2(y.x * scale, y.y * scale);
        }
    } else {
        const int rows = hop / ksum;
        const long r0 = seg * rows;
        const bool time_major = p.layout == TIME_MAJOR;
        float* const dst = time_major ? p.out + r0 * p.out_stride + chan : p.out + chan * p.out_stride + r0;
        const long step = time_major ? p.out_stride : 1;
        for (int r = tid; r < rows; r += T) {
            float acc = 0.0f;
            int i = lead + r * ksum;
            for (int q = 0; q < ksum; ++q, ++i) {
                const float2 y = tile[rowfft::place(i)];
                acc = acc + pfb::power(make_float2(y.x * scale, y.y * scale));
            }
            dst[r * step] = acc;
        }
    }
}

using Log2Ns = Vals<9, 10, 11, 12, 13, 14>;

hipError_t launch(int log2n, const Params& p, long nseg, int nchan, hipStream_t st)
{
    return pick(Log2Ns{}, log2n, [&](auto n) {
        return rtlws::launch(&cdd_kernel<decltype(n)::value>, dim3((unsigned)nseg, (unsigned)nchan), dim3((unsigned)threads_of(log2n)),
                             (size_t)lds_of(log2n), st, p);
    });
}

// asking for a kernel's attributes loads its code object: nothing is left to load under a capture
hipError_t prepare(int log2n, int device)
{
    return pick(Log2Ns{}, log2n, [&](auto n) {
        const hipError_t e = load_kernel(&cdd_kernel<decltype(n)::value>);
        return e != hipSuccess ? e : lds_opt_in(&cdd_kernel<decltype(n)::value>, device, (size_t)lds_of(log2n));
    });
}

}  // namespace cdd
}  // namespace rtlws

// cdd.h -- shared between cdd.hip (the kernel) and cdd_shim.hip (rtlws_cdd.h's host glue): the limits, what a run
// launches, the order of the plan's tables on the device and the kernel's arguments.
#ifndef RTLWS_CSRC_CDD_H
#define RTLWS_CSRC_CDD_H

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace rtlws {
namespace cdd {

constexpr int MIN_LOG2N = 9, MAX_LOG2N = 14, MAX_NCHAN = 1024, LANES = 64;
constexpr long MAX_NSEG = 1L << 20;                            // times 1024 threads: inside a launch's 2^32 threads an axis
constexpr int CHANNEL_MAJOR = 0, TIME_MAJOR = 1;

// One workgroup per (segment, channel): a thread per radix-16 butterfly of row_fft.h, a wavefront at least; the segment in
// one tile of rowfft::Shape<LOG2N>::TILE_F2 float2
constexpr int threads_of(int log2n) { return (1 << (log2n - 4)) < LANES ? LANES : 1 << (log2n - 4); }
constexpr int lds_of(int log2n) { return 8 * ((1 << log2n) + (1 << (log2n - 4))); }
static_assert(threads_of(9) == 64 && threads_of(14) == 1024 && lds_of(14) == 136 * 1024 && lds_of(9) == 4352, "the workgroup at the two ends");

// Where bin k lies after rowfft::forward, as a point index (rowfft::pos, restated for the host: the shim uploads H_c in
// this order, so that the kernel reads its table linearly; a table in another order fails every case of
// tests/test_cdd_gpu.py)
constexpr int pos_of(int log2n, int k)
{
    const int m = 1 << log2n;
    return log2n >= 12 ? (k & 15) * (m / 16) + ((k >> 4) & 15) * (m / 256) + ((k >> 8) & 15) * (m / 4096) + (k >> 12)
                       : (k & 15) * (m / 16) + ((k >> 4) & 15) * (m / 256) + (k >> 8);
}

struct Params {
    const float2* in;          // channel c at in + c * in_stride
    float* out;                // voltages (as float2) or power rows
    const float2* table;       // [nchan][N]: entry i of a channel is H_c[k], i = pos(k)
    const float2* tw;          // [N] e^(-2 pi i j / (2 N)): row_fft.h's
    long in_stride, out_stride;
    int lead, hop, ksum;       // ksum 0: voltages
    int layout;
    float scale;               // 1 / N
};

// a grid of nseg by nchan workgroups of threads_of(log2n) threads and lds_of(log2n) bytes
hipError_t launch(int log2n, const Params& p, long nseg, int nchan, hipStream_t st);
// the kernel of this log2n loaded on `device` (the current one) and its LDS limit raised above 64 KiB where it needs that
hipError_t prepare(int log2n, int device);

}  // namespace cdd
}  // namespace rtlws
#endif

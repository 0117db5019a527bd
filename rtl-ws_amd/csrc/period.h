// period.h -- shared between period.hip (the kernel) and period_shim.hip (rtlws_period.h's host glue): the limits, the
// workgroup a frame length takes and the kernel's arguments; and what the whole periodicity-search family
// takes from here (periodlong.h includes it): LANES, MAX_LEVELS, MIN_NORM, MIN_SEG and chunk_of.
#ifndef RTLWS_CSRC_PERIOD_H
#define RTLWS_CSRC_PERIOD_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rtlws {
namespace period {

constexpr int MIN_LOG2N = 10, MAX_LOG2N = 15, MAX_LEVELS = 5, MIN_NORM = 16, MIN_SEG = 64, MAX_TRIALS = 65536;

// One workgroup owns one trial: N = 2^log2n real samples packed as M = N / 2 complex points, a thread a radix-16
// butterfly of a pass (M / 16 of them), never fewer than one wavefront.  The tile is M float2 with one place of padding
// behind every 16 (row_fft.h): 136 KiB at log2n = 15.
constexpr int LANES = 64;
constexpr int threads_of(int log2n) { return (1 << (log2n - 5)) < LANES ? LANES : 1 << (log2n - 5); }
constexpr int lds_bytes(int log2n) { return 8 * ((1 << (log2n - 1)) + (1 << (log2n - 5))); }
static_assert(threads_of(10) == 64 && threads_of(11) == 64 && threads_of(12) == 128 && threads_of(15) == 1024, "a workgroup's threads");
static_assert(lds_bytes(15) == 136 * 1024 && lds_bytes(10) == 4352, "a workgroup's LDS");

// The k a wavefront walks before it reduces its lanes' peaks, of the `bins` bins a workgroup has in view (a trial's M
// here, a span of 16384 in periodlong.h): a segment, but never more than 1024 (so that every wavefront of a workgroup
// has a chunk), the partial peaks of a longer segment meeting in LDS
constexpr int chunk_of(int bins, int seg) { return seg < 1024 ? seg : bins < 1024 ? bins : 1024; }

struct Params {
    const float* in;
    float* best;
    int32_t* at;
    float* power;          // NULL: not written
    float* white;          // NULL: not written
    const float2* tw;      // [N / 2] e^(-2 pi i j / N)
    long in_stride;
    int nsamp, levels, log2norm, seg, klo;
    float norm_scale;      // 2^-log2norm
};

// ntrials workgroups
hipError_t launch_period(int log2n, const Params& p, int ntrials, hipStream_t st);
// loads the kernel of the frame length on `device` (the current one) and raises its LDS limit where it needs more than 64 KiB
hipError_t prepare_period(int log2n, int device);

}  // namespace period
}  // namespace rtlws
#endif

// periodlong.h -- shared between periodlong.hip (the kernels) and periodlong_shim.hip (rtlws_periodlong.h's host glue):
// the limits, the decomposition of a frame length, what every stage launches and the kernels' arguments.
#ifndef RTLWS_CSRC_PERIODLONG_H
#define RTLWS_CSRC_PERIODLONG_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "period.h"

namespace rtlws {
namespace periodlong {

// the family's own (period.h): the stages behind the transform are one text (period_stages.h)
using period::LANES;
using period::MAX_LEVELS;
using period::MIN_NORM;
using period::MIN_SEG;
using period::chunk_of;
constexpr int MIN_LOG2N = 16, MAX_LOG2N = 22, MAX_NORM = 16384, MAX_SEG = 16384, MAX_TRIALS = 65536;

// N = 2^log2n real samples are M = N / 2 complex points z[j] = y[2 j] + i y[2 j + 1], M = M1 M2, j = j1 M2 + j2,
// k = k1 + M1 k2: M1 = 16 up to log2n 19 and 256 above, M2 = 2^11 .. 2^14 the length of a row that row_fft.h transforms
constexpr int log2m1_of(int log2n) { return log2n <= 19 ? 4 : 8; }
constexpr int log2m2_of(int log2n) { return log2n - 1 - log2m1_of(log2n); }
static_assert(log2m2_of(16) == 11 && log2m2_of(19) == 14 && log2m2_of(20) == 11 && log2m2_of(22) == 13, "the rows' lengths");

// The stages, each one launch per group of trials; a workgroup's threads and LDS, and the workgroups of one trial
enum { STAGE_MEAN = 0, STAGE_COLS, STAGE_ROWS, STAGE_UNTANGLE, STAGE_WHITEN, STAGE_PEAKS, STAGES };
constexpr int MEAN_PARTS = 64, MEAN_THREADS = 256;         // a trial's samples in 64 stretches, one f64 sum each
constexpr int COLS_THREADS = 256, COLS256_TILE = 16;       // M1 = 16: a thread a column; M1 = 256: a workgroup 16 columns
constexpr int SPAN = 16384, SPAN_THREADS = 1024;           // whitening and peaks: a workgroup owns 16384 bins
constexpr int untangle_cols(int log2m1) { return log2m1 == 4 ? 64 : 16; }      // columns k2 of a tile; M1 times that many bins
constexpr int UNTANGLE_THREADS = 256;
constexpr int rows_threads(int log2m2) { return (1 << (log2m2 - 4)) < LANES ? LANES : 1 << (log2m2 - 4); }
constexpr int rows_lds(int log2m2) { return 8 * ((1 << log2m2) + (1 << (log2m2 - 4))); }
constexpr int cols_lds(int log2m1) { return log2m1 == 4 ? 0 : 8 * 256 * (COLS256_TILE + 1); }
constexpr int untangle_lds(int log2m1) { return 8 * 2 * (1 << log2m1) * (untangle_cols(log2m1) + 1); }
static_assert(rows_lds(14) == 136 * 1024 && untangle_lds(8) == 69632 && untangle_lds(4) == 16640, "the stages' LDS");

constexpr int stage_blocks(int stage, int log2n)
{
    const int l1 = log2m1_of(log2n), l2 = log2m2_of(log2n), m = 1 << (log2n - 1);
    return stage == STAGE_MEAN ? MEAN_PARTS
           : stage == STAGE_COLS ? (l1 == 4 ? (1 << l2) / COLS_THREADS : (1 << l2) / COLS256_TILE)
           : stage == STAGE_ROWS ? 1 << l1
           : stage == STAGE_UNTANGLE ? (1 << l2) / (2 * untangle_cols(l1))
                                     : m / SPAN;
}
constexpr int stage_threads(int stage, int log2n)
{
    return stage == STAGE_MEAN ? MEAN_THREADS
           : stage == STAGE_COLS ? COLS_THREADS
           : stage == STAGE_ROWS ? rows_threads(log2m2_of(log2n))
           : stage == STAGE_UNTANGLE ? UNTANGLE_THREADS
                                     : SPAN_THREADS;
}
constexpr int stage_lds(int stage, int log2n)
{
    return stage == STAGE_MEAN ? 8 * (MEAN_THREADS / LANES)
           : stage == STAGE_COLS ? cols_lds(log2m1_of(log2n))
           : stage == STAGE_ROWS ? rows_lds(log2m2_of(log2n))
           : stage == STAGE_UNTANGLE ? untangle_lds(log2m1_of(log2n))
           : stage == STAGE_WHITEN ? 4 * (SPAN_THREADS / LANES)
                                   : 8 * MAX_LEVELS * 16;
}

// A trial in flight takes M float2 (the transform, in place), M float (P, then W over it) and the mean's partial sums
constexpr size_t trial_bytes(int log2n) { return (size_t)12 * ((size_t)1 << (log2n - 1)) + 8 * MEAN_PARTS; }

struct Params {
    const float* in;       // the first trial of the group
    float* best;           // the caller's rows, from trial 0
    int32_t* at;
    float* power;          // NULL: not written
    float* white;          // NULL: not written
    float2* z;             // workspace [group][M]
    float* pw;             // workspace [group][M]: P, then W
    double* sums;          // workspace [group][MEAN_PARTS]
    const float2* tw;      // [M] e^(-2 pi i j / N): the untangling
    const float2* twist;   // [M1][M2] e^(-2 pi i k1 j2 / M)
    const float2* tw_row;  // [M2] e^(-2 pi i j / (2 M2)): row_fft.h's
    const float2* tw256;   // [256] e^(-2 pi i j / 256)
    long in_stride;
    int trial0;            // the group's first trial
    int log2n, nsamp, levels, log2norm, seg, klo;
    float norm_scale;      // 2^-log2norm
};

// the six launches of one group of `group` trials, in the stages' order: the head reads the caller's series (mean,
// columns) and the tail the workspace alone (rows .. peaks), so that a library with a head of its own (accel.hip) runs
// this tail behind it
hipError_t launch_head(const Params& p, int group, hipStream_t st);
hipError_t launch_tail(const Params& p, int group, hipStream_t st);
hipError_t launch_group(const Params& p, int group, hipStream_t st);
// loads every kernel of the frame length on `device` (the current one) and raises the LDS limits above 64 KiB
hipError_t prepare(int log2n, int device);

}  // namespace periodlong
}  // namespace rtlws
#endif

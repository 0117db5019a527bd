// accel.h -- shared between accel.hip (the kernels) and accel_shim.hip (rtlws_accel.h's host glue): the limits, the
// quadratic index map in integers -- one text for the host's rtlws_accel_shift and the kernels -- and the kernels'
// arguments.  The stages behind the columns are periodlong.hip's, linked as they are.
#ifndef RTLWS_CSRC_ACCEL_H
#define RTLWS_CSRC_ACCEL_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "periodlong.h"

namespace rtlws {
namespace accel {

constexpr int MAX_NACCEL = 1024, MAX_VIRTUAL = 65536;
constexpr int64_t MAX_COEF = (int64_t)1 << 40;             // |c| in units of 2^-64 samples per sample^2
constexpr int RESAMPLE_THREADS = 256, RESAMPLE_QUAD = 4;   // a thread four consecutive n, one 16-byte store

// s_c(n) = floor((c n (last - n) + 2^63) / 2^64), last = nsamp - 1, 0 <= n <= last < 2^22, |c| <= 2^40: exact, the floor
// towards -Inf, a half up for either sign of c.  With p = n (last - n) = p1 2^32 + p0 and c = ch 2^32 + cl (ch signed,
// cl, p0 unsigned 32 bits):  c p = (ch p0 + c p1) 2^32 + cl p0, so with A = ch p0 + c p1 + (cl p0 >> 32) (|A| < 2^52: no
// overflow)  c p + 2^63 = (A + 2^31) 2^32 + (cl p0 mod 2^32), and the quotient by 2^64 is (A + 2^31) >> 32, the shift
// arithmetic: the low 32 bits are a fraction below one of the unit the floor is taken in.
__host__ __device__ __forceinline__ int shift(int64_t c, int n, int last)
{
    const uint64_t p = (uint64_t)(uint32_t)n * (uint32_t)(last - n);
    const int64_t p0 = (int64_t)(p & 0xffffffffu), p1 = (int64_t)(p >> 32);
    const int64_t ch = c >> 32;
    const uint64_t cl = (uint64_t)c & 0xffffffffu;
    const int64_t a = ch * p0 + c * p1 + (int64_t)((cl * (uint64_t)p0) >> 32);
    return (int)((a + ((int64_t)1 << 31)) >> 32);
}

// The head of a group of virtual trials: periodlong's arguments (in: trial 0 of the caller's series; trial0: the
// group's first virtual trial v) and the table.  Virtual trial v = t naccel + a reads trial t through coefs[a].
struct Params {
    periodlong::Params s;
    const int64_t* coefs;  // [naccel], on the device
    int naccel;
};

struct ResampleParams {
    const float* in;       // trial 0
    float* out;            // row 0
    const int64_t* coefs;  // [naccel], on the device
    long in_stride, out_stride;
    int nsamp;
    int a_first, a_count;
    int rows;              // ntrials a_count
};

// mean and columns through the map, then periodlong.hip's tail: six launches
hipError_t launch_group(const Params& p, int group, hipStream_t st);
// one launch: row r = t a_count + (a - a_first) of the output
hipError_t launch_resample(const ResampleParams& p, hipStream_t st);
// workgroups of the resampling launch along x and y
constexpr int resample_blocks_x(int nsamp) { return (nsamp + RESAMPLE_QUAD * RESAMPLE_THREADS - 1) / (RESAMPLE_QUAD * RESAMPLE_THREADS); }
constexpr int resample_blocks_y(int rows) { return rows < 65535 ? rows : 65535; }
// loads every kernel of the frame length on `device` (the current one), periodlong.hip's among them
hipError_t prepare(int log2n, int device);

}  // namespace accel
}  // namespace rtlws
#endif

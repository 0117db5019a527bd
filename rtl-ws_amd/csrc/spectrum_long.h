// spectrum_long.h -- shared between spectrum_long.hip (the kernels) and long_shim.hip (rtlws_long.h's host glue).
#ifndef RTLWS_SPECTRUM_LONG_H
#define RTLWS_SPECTRUM_LONG_H

#include <cmath>
#include <vector>

#include "rtlws_internal.h"

namespace rtlws {
namespace lng {

// Four-step split of N = 2^m: N1 = 2^ceil(m/2) (pass A), N2 = 2^floor(m/2) (pass B), both 128 .. 1024.
constexpr int MIN_LOG2N = 14, MAX_LOG2N = 20;
constexpr int log2_n1(int m) { return (m + 1) / 2; }
constexpr int log2_n2(int m) { return m / 2; }

// A workgroup of 512 threads transforms a tile of 8192 points: T = 8192 / L columns of an L-point transform,
// sixteen points per thread, 128 KiB of LDS (one workgroup per CU, two wavefronts per SIMD).
constexpr int TILE_POINTS = 8192;
constexpr int THREADS = 512;
constexpr int LDS_BYTES = TILE_POINTS * 16;
constexpr int tile_cols(int log2l) { return TILE_POINTS >> log2l; }

// W_N^j from two short tables: j = 1024 h + l, W_N^j = twh[h] * twl[l]
constexpr int TW_SPLIT_LOG2 = 10;

enum { ROWS_F64 = 0, ROWS_F32 = 1, ROWS_U8 = 2 };

struct LongParams {
    const void* in;        // device: the group's frames
    void* out;             // device: the group's rows
    double2* ws;           // device: workspace, frame f at ws + f * N, element (k1, n2) at k1 * N2 + n2
    const double2* twc;    // [1024] W_1024^e: the sub-transforms' twiddles
    const double2* twl;    // [1024] W_N^l
    const double2* twh;    // [N / 1024] W_N^(1024 h)
    int log2n1, log2n2;
    int k_avg;
    int out_mode;          // OUT_*
    double lin_gain;       // 10^(gain_db/10), C integer division (src/cbb_main.c:112)
    double in_scale;       // 1/128 or 1
};

// The twiddle tables' entries (host): W_n^j, j < count * step, every step-th, evaluated in long double, rounded once
inline std::vector<double2> roots(long n, long step, int count)
{
    const long double two_pi = 6.283185307179586476925286766559005768L;
    std::vector<double2> w((size_t)count);
    for (int i = 0; i < count; ++i) {
        const long double a = -two_pi * (long double)(i * step) / (long double)n;
        w[(size_t)i] = make_double2((double)cosl(a), (double)sinl(a));
    }
    return w;
}

// pass A over `frames` frames, pass B over `rows` = frames / k_avg rows
hipError_t launch_long_pass_a(const LongParams&, int in_kind, long frames, hipStream_t);
hipError_t launch_long_pass_b(const LongParams&, int rows_kind, long rows, hipStream_t);
// raise the dynamic-LDS limit of the two kernels a plan launches (once per kernel and device)
hipError_t prepare_long(int log2n, int in_kind, int rows_kind, int device);

}  // namespace lng
}  // namespace rtlws
#endif

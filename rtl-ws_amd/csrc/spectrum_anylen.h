// spectrum_anylen.h -- shared between spectrum_anylen.hip (the kernels) and anylen_shim.hip (rtlws_anylen.h's glue).
#ifndef RTLWS_SPECTRUM_ANYLEN_H
#define RTLWS_SPECTRUM_ANYLEN_H

#include "spectrum_long.h"

namespace rtlws {
namespace anylen {

// Frame lengths served, and the convolution length M = 2^m >= 2 N - 1 they run at (never below the four-step
// transform's smallest size): m, or -1
constexpr int MIN_N = 2, MAX_N = 1 << 19;
constexpr int conv_log2(long n)
{
    if (n < MIN_N || n > MAX_N) return -1;
    int m = lng::MIN_LOG2N;
    while ((1L << m) < 2 * n - 1) ++m;
    return m;
}

struct AnyParams {
    const void* in;          // device: the group's frames, N samples each, no padding
    void* out;               // device: the group's rows, N values each
    double2* ws1;            // device: frame f at ws1 + f * M, element (k1, n2) at k1 * N2 + n2 (passes 1 -> 2, 3 -> 4)
    double2* ws2;            // device: frame f at ws2 + f * M, natural order k = k1 + N1 k2 (pass 2 -> 3)
    const double2* twc;      // [1024] W_1024^e: the sub-transforms' twiddles
    const double2* twl;      // [1024] W_M^l
    const double2* twh;      // [M / 1024] W_M^(1024 h)
    const double2* chirp;    // [N] w[n] = exp(-i pi n^2 / N)
    const double2* bhat;     // [M] FFT_M(b) / M, b[n] = conj(w[|n|]) wrapped around M; natural order
    int log2n1, log2n2;      // M = N1 * N2
    int n;                   // N
    int k_avg;
    int out_mode;            // OUT_*
    double lin_gain;         // 10^(gain_db/10), C integer division (src/cbb_main.c:112)
    double in_scale;         // 1/128 or 1
};

// The four launches of a group, in this order: `frames` frames, `rows` = frames / k_avg rows.
hipError_t launch_pass_a_in(const AnyParams&, int in_kind, long frames, hipStream_t);
hipError_t launch_pass_b_cplx(const AnyParams&, long frames, hipStream_t);
hipError_t launch_pass_a_ws(const AnyParams&, long frames, hipStream_t);
hipError_t launch_pass_b_pow(const AnyParams&, int rows_kind, long rows, hipStream_t);
// raise the dynamic-LDS limit of the four kernels a plan launches (once per kernel and device)
hipError_t prepare_anylen(int log2m, int in_kind, int rows_kind, int device);

}  // namespace anylen
}  // namespace rtlws
#endif

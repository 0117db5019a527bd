// fm_math.h -- the two f32 expressions of the FM receive chain, one text of each: shared by the stand-alone kernels
// (resample_kernels.hip: fm_demod_kernel, halfband_kernel) and the fused chain (fm_chain.hip).  Both files are
// built with -ffp-contract=off: multiply then add, never fma, for bit parity with an IEEE evaluation of the C source.
#ifndef RTLWS_FM_MATH_H
#define RTLWS_FM_MATH_H

#include <hip/hip_runtime.h>

namespace rtlws {

// atan2_approx of reference src/common_sp.h:40-76, evaluated as the C source
// reads under IEEE rules: f32 divide/multiply/add without contraction (this
// file is built with -ffp-contract=off), and the +-M_PI corrections as a
// double-precision add rounded back to f32.
__device__ __forceinline__ float atan2_approx_dev(float y, float x)
{
    const float pi_by_2 = (float)(3.14159265358979323846 / 2);
    const double pi_d = 3.14159265358979323846;
    if (x == 0.0f) {
        if (y > 0.0f) return pi_by_2;
        if (y == 0.0f) return 0.0f;
        return -pi_by_2;
    }
    const float z = __fdiv_rn(y, x);
    if (fabsf(z) < 1.0f) {
        const float at = __fdiv_rn(z, __fadd_rn(1.0f, __fmul_rn(__fmul_rn(0.28f, z), z)));
        if (x < 0.0f) {
            if (y < 0.0f) return (float)((double)at - pi_d);
            return (float)((double)at + pi_d);
        }
        return at;
    }
    const float at = __fsub_rn(pi_by_2, __fdiv_rn(z, __fadd_rn(__fmul_rn(z, z), 0.28f)));
    if (y < 0.0f) return (float)((double)at - pi_d);
    return at;
}

// reference src/audio_main.c:124-131: first difference of the phase, hard limit (scale == 1)
__device__ __forceinline__ float fm_limit_dev(float ph, float prev)
{
    float d = __fsub_rn(ph, prev);
    if (d > 1.0f) d = 1.0f;
    else if (d < -1.0f) d = -1.0f;
    return d;
}

// One output of the 11-tap half-band, reference src/resample.c:53-64: xk is the input k samples before the
// output's own (x[2n - k]); the centre tap first, then the even taps in the source's order.
__device__ __forceinline__ float halfband_dev(float x5, float x0, float x2, float x4, float x6, float x8, float x10)
{
    const float h0 = 0.01824f, h2 = -0.11614f, h4 = 0.34790f, h5 = 0.5f;   // src/resample.c:4
    float acc = __fmul_rn(h5, x5);                       // src/resample.c:57
    acc = __fadd_rn(acc, __fmul_rn(h0, x0));             // k = 0   src/resample.c:60-64
    acc = __fadd_rn(acc, __fmul_rn(h2, x2));             // k = 2
    acc = __fadd_rn(acc, __fmul_rn(h4, x4));             // k = 4
    acc = __fadd_rn(acc, __fmul_rn(h4, x6));             // k = 6
    acc = __fadd_rn(acc, __fmul_rn(h2, x8));             // k = 8
    acc = __fadd_rn(acc, __fmul_rn(h0, x10));            // k = 10
    return acc;
}

}  // namespace rtlws
#endif

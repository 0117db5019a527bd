// pfb_plan.h -- the host side of a polyphase plan: the transform's table and the prototype on the device.  The one
// text of pfb_shim.hip (librtlws_pfb.so) and pfbspec_shim.hip (librtlws_pfbspec.so): both plans hold the same bits.
#ifndef RTLWS_PFB_PLAN_H
#define RTLWS_PFB_PLAN_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

namespace rtlws {
namespace pfb {

// e^(-2 pi i j / M) in f64, rounded once; the quadrant points exactly
inline void build_twiddles(int k, float* re_im)
{
    const int M = 1 << k;
    for (int j = 0; j < M; ++j) {
        const double a = -2.0 * M_PI * (double)j / (double)M;
        double c = std::cos(a), s = std::sin(a);
        if ((4 * j) % M == 0) {
            c = std::rint(c);
            s = std::rint(s);
        }
        re_im[2 * j] = (float)c;
        re_im[2 * j + 1] = (float)s;
    }
}

inline void free_plan_arrays(int16_t* d_taps, float2* d_tw)
{
    if (d_taps) (void)hipFree(d_taps);
    if (d_tw) (void)hipFree(d_tw);
}

// The prototype (taps_per_branch * M int16 in host memory) and the table of build_twiddles on the current device.
// On failure nothing stays allocated and both pointers are null.
inline hipError_t upload_plan_arrays(int k, int taps_per_branch, const int16_t* taps, int16_t** d_taps, float2** d_tw)
{
    const size_t M = (size_t)1 << k, ntaps = M * (size_t)taps_per_branch;
    std::vector<float> tw(2 * M);
    build_twiddles(k, tw.data());
    *d_taps = nullptr;
    *d_tw = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(d_taps), ntaps * sizeof(int16_t));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(d_tw), tw.size() * sizeof(float));
    if (err == hipSuccess) err = hipMemcpy(*d_taps, taps, ntaps * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(*d_tw, tw.data(), tw.size() * sizeof(float), hipMemcpyHostToDevice);
    if (err != hipSuccess) {
        free_plan_arrays(*d_taps, *d_tw);
        *d_taps = nullptr;
        *d_tw = nullptr;
    }
    return err;
}

}  // namespace pfb
}  // namespace rtlws
#endif

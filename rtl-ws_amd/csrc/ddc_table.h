// ddc_table.h -- the phasor table T of include/rtlws_ddc.h, one builder text for every library that holds a copy
// (ddc_plan.h's open_plan, rtlws_ddc_table).  Host only, and no header but the standard library's: tests/test_fmbank_cpu.py
// compiles it alone.
#ifndef RTLWS_DDC_TABLE_H
#define RTLWS_DDC_TABLE_H

#include <cmath>
#include <cstdint>

namespace rtlws {
namespace ddc {

// t[2 j], t[2 j + 1] for j < P (a multiple of four): T[j] = rint(2^14 (cos, sin)(2 pi j / P)) from the exact integer
// phase j, the axis values exact (as twiddle_tables.cpp's W()); no entry lies closer than 8.7e-7 to a rounding tie, a
// double's cos and sin are 1e-12 off
inline void build_table(int16_t* t, int P)
{
    const double two_pi = 6.283185307179586476925286766559;
    for (int j = 0; j < P; ++j) {
        double c, s;
        if (j == 0) c = 1, s = 0;
        else if (j == P / 4) c = 0, s = 1;
        else if (j == P / 2) c = -1, s = 0;
        else if (j == 3 * (P / 4)) c = 0, s = -1;
        else c = std::cos(two_pi * j / P), s = std::sin(two_pi * j / P);
        t[2 * j] = (int16_t)std::lrint(16384.0 * c);
        t[2 * j + 1] = (int16_t)std::lrint(16384.0 * s);
    }
}

}  // namespace ddc
}  // namespace rtlws
#endif

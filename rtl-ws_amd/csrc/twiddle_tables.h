// twiddle_tables.h -- the host-side twiddle and window tables of the spectrum kernels.
//
// Host-only (no HIP): shim.hip uploads what these functions return once per engine and N;
// tests/test_tables_cpu.py builds the unit with g++ and holds the tables bit for bit.
#ifndef RTLWS_TWIDDLE_TABLES_H
#define RTLWS_TWIDDLE_TABLES_H

#include <vector>

namespace rtlws {

// the layout of float2 / double2
template <typename T> struct Pair { T x, y; };
using F2 = Pair<float>;
using D2 = Pair<double>;

// One size's tables.  tables_f32 fills the first five, tables_f64 the rest; a table the size
// has no kernel for stays empty.
struct HostTables {
    std::vector<F2> tw1;        // fused: [T][16] W_N^(t*rev16(s)); direct: [N] W_N^k
    std::vector<F2> tw1_128;    // fused: tw1 / 128 (u8, s32, CIC input)
    std::vector<F2> tw2;        // fused: [16][R3/2] last-pass (cos, sin/cos) pairs
    std::vector<F2> hann_cs;    // fused: [T] (0.5 cos, 0.5 sin)(2 pi t / N)
    std::vector<float> hann;    // [N] periodic Hann
    std::vector<D2> tw64;       // spectrum_f64.hip: [N] W_N^k
    std::vector<double> hann64; //   [N] periodic Hann
    std::vector<D2> tw1_64;     // spectrum_f64_fused.hip: [T][16] W_N^(t*rev16(s)) / 128
    std::vector<D2> tw1u_64;    //   ... unscaled (real f32 input)
    std::vector<D2> tw2_64;     //   [16][R3/2] last-pass (cos, sin/cos) pairs
    std::vector<D2> hann_cs64;  //   [T] (0.5 cos, 0.5 sin)(2 pi t / N)
    std::vector<D2> twxa_64;    // spectrum_f64_1024x.hip (N = 1024): [4][8] pass-A (cos, tan) pairs
    std::vector<D2> twxb_64;    //   [64][16] inner twiddles x lane constant / 128
};

bool is_fused_n(int n);

// evaluated in double, rounded once to float; fused tables for is_fused_n(n_fft), direct ones otherwise
HostTables tables_f32(int n_fft);
// evaluated in long double, rounded once to double; fused and 1024x tables where those kernels exist
HostTables tables_f64(int n_fft);

}  // namespace rtlws

#endif  // RTLWS_TWIDDLE_TABLES_H

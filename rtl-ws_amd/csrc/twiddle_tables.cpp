// twiddle_tables.cpp -- see twiddle_tables.h.  Every table is a unit root W(num, den) of the
// working precision (double for the f32 kernels, long double for the f64 ones), rounded once.
#include "twiddle_tables.h"

#include <cmath>

namespace rtlws {
namespace {

template <typename T> struct Prec;
template <> struct Prec<double> {
    static constexpr double two_pi = 6.283185307179586476925286766559;
    static constexpr double tiny = 1e-20;
};
template <> struct Prec<long double> {
    static constexpr long double two_pi = 6.283185307179586476925286766559005768L;
    static constexpr long double tiny = 1e-20L;
};

// exp(-2 pi i num/den), straight from cos / sin
template <typename T> Pair<T> W_libm(long num, long den)
{
    const T a = -Prec<T>::two_pi * (T)num / (T)den;
    return {std::cos(a), std::sin(a)};
}

// exp(-2 pi i num/den) with the axis values exact
template <typename T> Pair<T> W(long num, long den)
{
    num %= den;
    if (num == 0) return {1, 0};
    if (4 * num == den) return {0, -1};
    if (2 * num == den) return {-1, 0};
    if (4 * num == 3 * den) return {0, 1};
    return W_libm<T>(num, den);
}

template <typename R, typename T> Pair<R> round_pair(Pair<T> w, T scale = 1)
{
    return {(R)(w.x * scale), (R)(w.y * scale)};
}

int rev16(int s) { return 4 * (s & 3) + (s >> 2); }

// The (cos, sin/cos) pairs fft_last<R> multiplies by for alpha = W_D^q (spectrum_fused.hip, "last
// pass"): for sub-size L = 2, 4, .. R and p < max(1, L/4), alpha^(R/L) * W_L^p = W_(D*L)^(q*R + p*D);
// cos = 0 is stored as 1e-20.
template <typename R, typename T> void last_pass_pairs(std::vector<Pair<R>>& out, long q, long D, int Rn)
{
    for (int L = 2; L <= Rn; L *= 2)
        for (int p = 0; p < (L >= 4 ? L / 4 : 1); ++p) {
            Pair<T> w = W<T>(q * Rn + (long)p * D, D * L);
            if (w.x == 0) w.x = Prec<T>::tiny;
            out.push_back({(R)w.x, (R)(w.y / w.x)});
        }
}

// The tables of the fused kernels (T = N/16 lanes, R3 = N/256): [T][16] W_N^(t*rev16(s)) through
// `w`, [16][R3/2] last-pass pairs of W_T^q2, [T] 0.5 W_N^-t (the generated Hann's lane constants).
template <typename R, typename T, typename Tw1>
void fused_tables(int n, Tw1 w, std::vector<Pair<R>>& tw2, std::vector<Pair<R>>& hann_cs)
{
    const int nt = n / 16, r3 = n / 256;
    for (int t = 0; t < nt; ++t)
        for (int s = 0; s < 16; ++s) w(t * 16 + s, (long)t * rev16(s));
    for (int q2 = 0; q2 < 16; ++q2) last_pass_pairs<R, T>(tw2, q2, nt, r3);
    for (int t = 0; t < nt; ++t) hann_cs.push_back(round_pair<R>(W<T>(-t, n), (T)0.5));
}

}  // namespace

bool is_fused_n(int n) { return n == 1024 || n == 2048 || n == 4096; }

HostTables tables_f32(int n)
{
    HostTables h;
    if (is_fused_n(n)) {
        h.tw1.resize((size_t)n), h.tw1_128.resize((size_t)n);
        fused_tables<float, double>(n, [&](int i, long e) {
            // no exact axes in this table: W_N^(N/4) keeps its 6.1e-17, as the f32 kernels were validated with
            h.tw1[i] = round_pair<float>(W_libm<double>(e % n, n));
            h.tw1_128[i] = {h.tw1[i].x * 0.0078125f, h.tw1[i].y * 0.0078125f};
        }, h.tw2, h.hann_cs);
    } else {
        for (int k = 0; k < n; ++k) h.tw1.push_back(round_pair<float>(W_libm<double>(k, n)));   // as above
    }
    for (int k = 0; k < n; ++k) h.hann.push_back((float)(0.5 - 0.5 * W_libm<double>(k, n).x));
    return h;
}

HostTables tables_f64(int n)
{
    typedef long double LD;
    HostTables h;
    for (int k = 0; k < n; ++k) {
        h.tw64.push_back(round_pair<double>(W<LD>(k, n)));
        h.hann64.push_back((double)(0.5L - 0.5L * W_libm<LD>(k, n).x));
    }
    if (!is_fused_n(n)) return h;
    // the f32 fused kernel's tables in long double; the u8 input scale 1/128 folded into tw1 (exact)
    h.tw1_64.resize((size_t)n), h.tw1u_64.resize((size_t)n);
    fused_tables<double, LD>(n, [&](int i, long e) {
        h.tw1_64[i] = round_pair<double>(W<LD>(e, n), 0.0078125L);
        h.tw1u_64[i] = round_pair<double>(W<LD>(e, n));
    }, h.tw2_64, h.hann_cs64);
    if (n == 1024) {
        // spectrum_f64_1024x.hip: 1024 = 4 x 16 x 16.  Pass A (radix-16 over r on lane (p, c)) absorbs
        // the geometric part (W_64^p)^r of the twiddle W_1024^(p (c + 16 r)): fft_last<16>'s pairs of
        // alpha = W_64^p.  The inner twiddles W_256^(c q) carry the lane constant W_1024^(p c) and the exact 1/128.
        for (int p = 0; p < 4; ++p) last_pass_pairs<double, LD>(h.twxa_64, p, 64, 16);
        for (int t = 0; t < 64; ++t)
            for (int s = 0; s < 16; ++s)
                h.twxb_64.push_back(round_pair<double>(W<LD>((long)(t & 15) * (4 * rev16(s) + (t >> 4)), 1024), 0.0078125L));
    }
    return h;
}

}  // namespace rtlws

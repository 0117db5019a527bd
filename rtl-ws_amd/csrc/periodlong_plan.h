// periodlong_plan.h -- what the glue of the two libraries over periodlong.hip's stages says the same way
// (periodlong_shim.hip, accel_shim.hip): the plan's rules, each worded once, the tables of a frame length, the trials a
// workspace holds in flight and the kernels' arguments over a plan's tables and workspace.  Internal linkage, like
// shim_common.h: a library has one shim.
#ifndef RTLWS_CSRC_PERIODLONG_PLAN_H
#define RTLWS_CSRC_PERIODLONG_PLAN_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <vector>

#include "periodlong.h"
#include "rtlws_periodlong.h"

namespace {

namespace pl = rtlws::periodlong;

static_assert(pl::MIN_LOG2N == RTLWS_PERIODLONG_MIN_LOG2N && pl::MAX_LOG2N == RTLWS_PERIODLONG_MAX_LOG2N &&
                  pl::MAX_LEVELS == RTLWS_PERIODLONG_MAX_LEVELS && pl::MIN_NORM == RTLWS_PERIODLONG_MIN_NORM &&
                  pl::MAX_NORM == RTLWS_PERIODLONG_MAX_NORM && pl::MIN_SEG == RTLWS_PERIODLONG_MIN_SEG && pl::MAX_SEG == RTLWS_PERIODLONG_MAX_SEG &&
                  pl::MAX_TRIALS == RTLWS_PERIODLONG_MAX_TRIALS && pl::STAGES == RTLWS_PERIODLONG_STAGES,
              "rtlws_periodlong.h and periodlong.h disagree");
static_assert(pl::trial_bytes(pl::MAX_LOG2N) <= RTLWS_PERIODLONG_WORKSPACE_CAP, "the cap holds a trial of every frame length");

[[maybe_unused]] const char* const NULL_PLAN = "null plan (no usable HIP device: there is no CPU path)";

[[maybe_unused]] bool power_of_two(int v) { return v > 0 && !(v & (v - 1)); }

[[maybe_unused]] int log2_of(int v)
{
    int l = 0;
    while ((1 << l) < v) ++l;
    return l;
}

// ---- the rules, each worded once ----
[[maybe_unused]] const char* why_not_plan(int log2n, int levels, int norm, int seg, int klo)
{
    if (log2n < pl::MIN_LOG2N || log2n > pl::MAX_LOG2N) return "log2n must be 16 .. 22";
    const int m = 1 << (log2n - 1);
    if (levels < 1 || levels > pl::MAX_LEVELS) return "levels must be 1 .. 5";
    if (norm < pl::MIN_NORM || norm > pl::MAX_NORM || !power_of_two(norm)) return "norm must be a power of two 16 .. 16384";
    if (seg < pl::MIN_SEG || seg > pl::MAX_SEG || !power_of_two(seg)) return "seg must be a power of two 64 .. 16384";
    if (klo < 1 || klo > m - 1) return "klo must be 1 .. N / 2 - 1";
    return nullptr;
}

[[maybe_unused]] const char* why_not_ntrials(int ntrials)
{
    return ntrials < 1 || ntrials > pl::MAX_TRIALS ? "ntrials must be 1 .. 65536" : nullptr;
}

// e^(-2 pi i k / N), k < N, every entry the exact root rounded once to f32: one octant evaluated in long double, the
// rest by the circle's symmetries, so that the axis values are exact and mirrored entries agree bit for bit
struct Roots {
    int n;
    std::vector<float> c, s;   // cos, sin (2 pi r / N), r <= N / 8
    explicit Roots(int n_) : n(n_), c((size_t)n_ / 8 + 1), s((size_t)n_ / 8 + 1)
    {
        const long double step = 6.283185307179586476925286766559L / (long double)n;
        for (int r = 0; r <= n / 8; ++r) c[r] = (float)cosl(step * r), s[r] = (float)sinl(step * r);
    }
    float2 operator()(long k) const
    {
        const int quarter = n / 4, q = (int)(k / quarter), r = (int)(k % quarter);
        const float co = r <= n / 8 ? c[r] : s[quarter - r], si = r <= n / 8 ? s[r] : c[quarter - r];
        // e^(-i theta) = (co, -si), times (-i)^q
        return q == 0 ? make_float2(co, -si) : q == 1 ? make_float2(-si, -co) : q == 2 ? make_float2(-co, si) : make_float2(si, co);
    }
};

// the tables of a frame length in the order a plan keeps them: tw [M], twist [M1][M2], tw_row [M2], tw256 [256]
[[maybe_unused]] std::vector<float2> host_tables(int log2n)
{
    const int n = 1 << log2n, m = n / 2, l1 = pl::log2m1_of(log2n), m1 = 1 << l1, m2 = m >> l1;
    std::vector<float2> t((size_t)2 * m + m2 + 256);
    const Roots root(n);
    float2* const tw = t.data();
    float2* const twist = tw + m;
    float2* const tw_row = twist + m;
    float2* const tw256 = tw_row + m2;
    for (int j = 0; j < m; ++j) tw[j] = root(j);
    for (int k1 = 0; k1 < m1; ++k1)
        for (int j2 = 0; j2 < m2; ++j2) twist[(size_t)k1 * m2 + j2] = root(2L * k1 * j2);      // k1 j2 < M
    for (int j = 0; j < m2; ++j) tw_row[j] = root((long)j * m1);
    for (int j = 0; j < 256; ++j) tw256[j] = root((long)j * (n / 256));
    return t;
}

// the trials in flight: what the caller expects, what the cap holds, what a launch's second grid axis takes
[[maybe_unused]] int in_flight(int log2n, int max_trials)
{
    size_t group = RTLWS_PERIODLONG_WORKSPACE_CAP / pl::trial_bytes(log2n);
    if (group > 65535) group = 65535;
    if (group > (size_t)max_trials) group = (size_t)max_trials;
    return (int)group;
}

// the kernels' arguments that a plan decides: its tables, its workspace of `group` trials and its parameters; the
// caller's pointers, in, in_stride, nsamp and trial0 are the run's
[[maybe_unused]] pl::Params plan_params(int log2n, int levels, int log2norm, int seg, int klo, int group, float2* d_tables, char* d_ws)
{
    const size_t m = (size_t)1 << (log2n - 1), m2 = m >> pl::log2m1_of(log2n);
    pl::Params kp{};
    kp.z = reinterpret_cast<float2*>(d_ws);
    kp.pw = reinterpret_cast<float*>(d_ws + (size_t)group * m * sizeof(float2));
    kp.sums = reinterpret_cast<double*>(d_ws + (size_t)group * m * (sizeof(float2) + sizeof(float)));
    kp.tw = d_tables;
    kp.twist = d_tables + m;
    kp.tw_row = d_tables + 2 * m;
    kp.tw256 = d_tables + 2 * m + m2;
    kp.log2n = log2n;
    kp.levels = levels;
    kp.log2norm = log2norm;
    kp.seg = seg;
    kp.klo = klo;
    kp.norm_scale = std::ldexp(1.0f, -log2norm);
    return kp;
}

}  // namespace
#endif

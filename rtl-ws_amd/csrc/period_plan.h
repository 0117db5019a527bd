// period_plan.h -- the host side the periodicity-search family shares (period_shim.hip, periodlong_shim.hip,
// accel_shim.hip): the rules of a run, each worded once and returning its text or nullptr, the period
// of a bin, and for the two libraries over periodlong.hip's stages the plan their opaque plan types derive from, with
// its rules, tables, open, close and the groups of a run.  Internal linkage, like shim_common.h: a library has one shim.
#ifndef RTLWS_CSRC_PERIOD_PLAN_H
#define RTLWS_CSRC_PERIOD_PLAN_H

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "period.h"
#include "periodlong.h"
#include "rtlws_periodlong.h"
#include "search_plan.h"

namespace rtlws {
namespace periodlong {

// What the two libraries over periodlong.hip's stages keep on the engine's device: rtlws_periodlong_plan is this,
// rtlws_accel_plan adds its table of coefficients
struct Plan {
    rtlws_engine* engine;
    int device;
    int log2n, levels, log2norm, seg, klo;
    int group;                 // trials in flight
    size_t ws_bytes;
    float2* d_tables;          // tw [M], twist [M], tw_row [M2], tw256 [256]
    char* d_ws;                // z [group][M] float2, pw [group][M] float, sums [group][64] double
};

}  // namespace periodlong
}  // namespace rtlws

namespace {

namespace pl = rtlws::periodlong;

static_assert(pl::MIN_LOG2N == RTLWS_PERIODLONG_MIN_LOG2N && pl::MAX_LOG2N == RTLWS_PERIODLONG_MAX_LOG2N &&
                  pl::MAX_LEVELS == RTLWS_PERIODLONG_MAX_LEVELS && pl::MIN_NORM == RTLWS_PERIODLONG_MIN_NORM &&
                  pl::MAX_NORM == RTLWS_PERIODLONG_MAX_NORM && pl::MIN_SEG == RTLWS_PERIODLONG_MIN_SEG && pl::MAX_SEG == RTLWS_PERIODLONG_MAX_SEG &&
                  pl::MAX_TRIALS == RTLWS_PERIODLONG_MAX_TRIALS && pl::STAGES == RTLWS_PERIODLONG_STAGES,
              "rtlws_periodlong.h and periodlong.h disagree");
static_assert(pl::trial_bytes(pl::MAX_LOG2N) <= RTLWS_PERIODLONG_WORKSPACE_CAP, "the cap holds a trial of every frame length");
static_assert(pl::MAX_TRIALS == rtlws::period::MAX_TRIALS && pl::MAX_TRIALS == rtlws::search::MAX_TRIALS, "one rule of ntrials for the series");

// the rule of ntrials and log2_of are search_plan.h's, which words them for every library over the dedispersed series
using rtlws::search::log2_of;
using rtlws::search::why_not_ntrials;

[[maybe_unused]] bool power_of_two(int v) { return v > 0 && !(v & (v - 1)); }

// ---- the family's rules, each worded once ----
// what every run refuses first: the trials, nsamp against the library's largest frame (why_nsamp words that limit), the
// stride
[[maybe_unused]] const char* why_not_input(int ntrials, int nsamp, int max_log2n, const char* why_nsamp, long in_stride)
{
    if (const char* why = why_not_ntrials(ntrials)) return why;
    if (nsamp < 1 || nsamp > (1 << max_log2n)) return why_nsamp;
    if (in_stride < nsamp) return "in_stride must be >= nsamp";
    if (in_stride % 4) return "in_stride must be a multiple of 4";
    return nullptr;
}

// ... and then, still without a plan: the pointers a search needs and the alignment of all five
[[maybe_unused]] const char* why_not_run(int ntrials, int nsamp, int max_log2n, const char* why_nsamp, long in_stride, const float* d_in,
                                         const float* d_best, const int32_t* d_at, const float* d_power, const float* d_white)
{
    if (const char* why = why_not_input(ntrials, nsamp, max_log2n, why_nsamp, in_stride)) return why;
    if (!d_in || !d_best || !d_at) return "null pointer";
    if (reinterpret_cast<uintptr_t>(d_in) & 15u) return "d_in must be 16-byte aligned";
    if (reinterpret_cast<uintptr_t>(d_best) & 3u) return "d_best must be 4-byte aligned";
    if (reinterpret_cast<uintptr_t>(d_at) & 3u) return "d_at must be 4-byte aligned";
    if (reinterpret_cast<uintptr_t>(d_power) & 3u) return "d_power must be 4-byte aligned";
    if (reinterpret_cast<uintptr_t>(d_white) & 3u) return "d_white must be 4-byte aligned";
    return nullptr;
}

// rtlws_*_samples: the period in samples of bin k at a level, 2^level N / k; why_log2n is the library's verdict on log2n
[[maybe_unused]] double samples(const char* fn, const char* why_log2n, int log2n, int level, int k)
{
    g_err.clear();
    if (why_log2n) return fail(fn, why_log2n, 0);
    if (level < 0 || level >= rtlws::period::MAX_LEVELS) return fail(fn, "level must be 0 .. 4", 0);
    if (k < 1 || k > (1 << (log2n - 1)) - 1) return fail(fn, "k must be 1 .. N / 2 - 1", 0);
    return (double)(1L << (log2n + level)) / (double)k;
}

// ---- the long frames: periodlong_shim.hip and accel_shim.hip ----
[[maybe_unused]] const char* const WHY_LONG_LOG2N = "log2n must be 16 .. 22";
[[maybe_unused]] const char* const WHY_LONG_NSAMP = "nsamp must be 1 .. 4194304";

[[maybe_unused]] const char* why_not_long_log2n(int log2n) { return log2n < pl::MIN_LOG2N || log2n > pl::MAX_LOG2N ? WHY_LONG_LOG2N : nullptr; }

[[maybe_unused]] const char* why_not_long_plan(int log2n, int levels, int norm, int seg, int klo)
{
    if (const char* why = why_not_long_log2n(log2n)) return why;
    const int m = 1 << (log2n - 1);
    if (levels < 1 || levels > pl::MAX_LEVELS) return "levels must be 1 .. 5";
    if (norm < pl::MIN_NORM || norm > pl::MAX_NORM || !power_of_two(norm)) return "norm must be a power of two 16 .. 16384";
    if (seg < pl::MIN_SEG || seg > pl::MAX_SEG || !power_of_two(seg)) return "seg must be a power of two 64 .. 16384";
    if (klo < 1 || klo > m - 1) return "klo must be 1 .. N / 2 - 1";
    return nullptr;
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

template <typename PlanT>
void close_plan(PlanT* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) {
        (void)hipFree(p->d_tables);
        (void)hipFree(p->d_ws);
    }
    delete p;
}

// rtlws_*_open of plan type PlanT (derived from pl::Plan): `why` is the verdict of the library's own rules on everything
// but max_trials.  The tables go to the engine's device, then more(plan) uploads what the library adds to the plan, then
// the workspace is allocated and the kernels of the frame length are loaded, the order of the libraries' own opens before
// they shared this one.  Whatever fails, the text is recorded and close(plan), the
// library's own rtlws_*_close, frees what there is: the plan starts zeroed, so a pointer never allocated is null there.
template <typename PlanT, typename More, typename Close>
PlanT* open_plan(const char* fn, const char* why, rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int max_trials, More&& more,
                 Close&& close)
{
    g_err.clear();
    if (!why && max_trials < 1) why = "max_trials must be >= 1";
    const int device = open_device(fn, why, e);
    if (device < 0) return nullptr;
    const std::vector<float2> t = host_tables(log2n);
    const int group = in_flight(log2n, max_trials);
    PlanT* p = new PlanT{};
    static_cast<pl::Plan&>(*p) = pl::Plan{e, device, log2n, levels, log2_of(norm), seg, klo, group, (size_t)group * pl::trial_bytes(log2n), nullptr, nullptr};
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&p->d_tables), t.size() * sizeof(float2));
    if (err == hipSuccess) err = hipMemcpy(p->d_tables, t.data(), t.size() * sizeof(float2), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = more(*p);
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&p->d_ws), p->ws_bytes);
    if (err == hipSuccess) err = pl::prepare(log2n, device);
    if (err != hipSuccess) {
        fail_hip(fn, "the tables, the workspace or the kernels", err);
        close(p);
        return nullptr;
    }
    return p;
}

// the kernels' arguments of a run: the plan's tables, its workspace of `group` trials and its parameters, the caller's
// rows, stride and nsamp; in and trial0 are a group's
[[maybe_unused]] pl::Params run_params(const pl::Plan& p, const float* d_in, long in_stride, int nsamp, float* d_best, int32_t* d_at,
                                       float* d_power, float* d_white)
{
    const size_t m = (size_t)1 << (p.log2n - 1), m2 = m >> pl::log2m1_of(p.log2n);
    pl::Params kp{};
    kp.in = d_in;
    kp.best = d_best;
    kp.at = d_at;
    kp.power = d_power;
    kp.white = d_white;
    kp.z = reinterpret_cast<float2*>(p.d_ws);
    kp.pw = reinterpret_cast<float*>(p.d_ws + (size_t)p.group * m * sizeof(float2));
    kp.sums = reinterpret_cast<double*>(p.d_ws + (size_t)p.group * m * (sizeof(float2) + sizeof(float)));
    kp.tw = p.d_tables;
    kp.twist = p.d_tables + m;
    kp.tw_row = p.d_tables + 2 * m;
    kp.tw256 = p.d_tables + 2 * m + m2;
    kp.in_stride = in_stride;
    kp.log2n = p.log2n;
    kp.nsamp = nsamp;
    kp.levels = p.levels;
    kp.log2norm = p.log2norm;
    kp.seg = p.seg;
    kp.klo = p.klo;
    kp.norm_scale = std::ldexp(1.0f, -p.log2norm);
    return kp;
}

// the groups of `total` trials that fit the workspace, one after the other: launch(first trial, trials) each
template <typename Launch>
hipError_t for_groups(const pl::Plan& p, int total, Launch&& launch)
{
    for (int t0 = 0; t0 < total; t0 += p.group) {
        const hipError_t err = launch(t0, total - t0 < p.group ? total - t0 : p.group);
        if (err != hipSuccess) return err;
    }
    return hipSuccess;
}

}  // namespace
#endif

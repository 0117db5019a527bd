// accel_shim.hip -- extern "C" glue of include/rtlws_accel.h (librtlws_accel.so) over the family's rules and long-frame
// plan (period_plan.h): the table's rules, the plan with the table of coefficients added, the groups of virtual trials
// of a run, and the host helpers of the map.  The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and
// nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "accel.h"
#include "period_plan.h"
#include "rtlws_accel.h"

// The family's long-frame plan (period_plan.h) and the coefficients on the engine's device
struct rtlws_accel_plan : rtlws::periodlong::Plan {
    int naccel;
    int64_t* d_coefs;          // [naccel]
};

namespace {

using namespace rtlws::accel;
typedef unsigned __int128 u128;

static_assert(MAX_NACCEL == RTLWS_ACCEL_MAX_NACCEL && MAX_COEF == RTLWS_ACCEL_MAX_COEF && MAX_VIRTUAL == RTLWS_ACCEL_MAX_VIRTUAL &&
                  pl::STAGES == RTLWS_ACCEL_STAGES && MAX_VIRTUAL == pl::MAX_TRIALS,
              "rtlws_accel.h and accel.h disagree");

const char* const WHY_VIRTUAL = "ntrials * naccel must be at most 65536";

// periodlong's rules, then naccel, the table, its entries in order
const char* why_not_table(int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs)
{
    if (const char* why = why_not_long_plan(log2n, levels, norm, seg, klo)) return why;
    if (naccel < 1 || naccel > MAX_NACCEL) return "naccel must be 1 .. 1024";
    if (!coefs) return "null table of coefficients";
    for (int a = 0; a < naccel; ++a)
        if (coefs[a] < -MAX_COEF || coefs[a] > MAX_COEF) return "every coefficient must be -2^40 .. 2^40";
    return nullptr;
}

int bits_of(u128 v)
{
    int bits = 0;
    for (; v; v >>= 1) ++bits;
    return bits;
}

// The integer nearest m 2^e / d, a half away from zero, exactly, for m < 2^106 and 1 <= d < 2^45; 2^41 where it is
// 2^41 or more (the callers' limit is 2^40)
uint64_t nearest(u128 m, long e, uint64_t d)
{
    const uint64_t beyond = (uint64_t)1 << 41;
    if (m == 0) return 0;
    u128 num = m, den = d;
    if (e >= 0) {
        if (bits_of(m) + e > 90) return beyond;              // m 2^e / d >= 2^(90 - 45) = 2^45
        num <<= e;
    } else {
        if (bits_of(d) - e > 126) return 0;                  // the divisor is 2^126 or more, above 2 m: not near a half
        den <<= -e;
    }
    u128 q = num / den;
    if (2 * (num - q * den) >= den) ++q;
    return q >= beyond ? beyond : (uint64_t)q;
}

// the integer nearest x y 2^e2 / d for finite doubles x, y, exactly; 0 with `beyond` set where it leaves +-2^40
int64_t scaled(double x, double y, int e2, uint64_t d, bool& beyond)
{
    // |x y| = mx my 2^(ex + ey - 106), mx and my integers below 2^53
    int ex = 0, ey = 0;
    const double fx = std::frexp(std::fabs(x), &ex), fy = std::frexp(std::fabs(y), &ey);
    const u128 m = (u128)(uint64_t)std::ldexp(fx, 53) * (uint64_t)std::ldexp(fy, 53);
    const uint64_t q = nearest(m, (long)ex + ey - 106 + e2, d);
    beyond = q > (uint64_t)MAX_COEF;
    return beyond ? 0 : (x < 0) != (y < 0) ? -(int64_t)q : (int64_t)q;
}

}  // namespace

extern "C" {

const char* rtlws_accel_last_error(void) { return g_err.c_str(); }

int rtlws_accel_supported(int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs)
{
    return supported("rtlws_accel", why_not_table(log2n, levels, norm, seg, klo, naccel, coefs));
}

int rtlws_accel_geometry(int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs, int ntrials, int* blocks,
                         int* threads, int* lds, int* nseg)
{
    const char* fn = "rtlws_accel_geometry";
    g_err.clear();
    if (const char* why = why_not_table(log2n, levels, norm, seg, klo, naccel, coefs)) return fail(fn, why, -1);
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if ((long)ntrials * naccel > MAX_VIRTUAL) return fail(fn, WHY_VIRTUAL, -1);
    for (int st = 0; st < pl::STAGES; ++st) {
        if (blocks) blocks[st] = pl::stage_blocks(st, log2n) * ntrials * naccel;     // at most 512 * 65536
        if (threads) threads[st] = pl::stage_threads(st, log2n);
        if (lds) lds[st] = pl::stage_lds(st, log2n);
    }
    if (nseg) *nseg = (1 << (log2n - 1)) / seg;
    return 0;
}

void rtlws_accel_close(rtlws_accel_plan* p)
{
    if (p && hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_coefs);
    close_plan(p);
}

rtlws_accel_plan* rtlws_accel_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo, int naccel, const int64_t* coefs,
                                   int max_trials)
{
    const auto upload = [&](rtlws_accel_plan& p) {
        p.naccel = naccel;
        const hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.d_coefs), (size_t)naccel * sizeof(int64_t));
        return err != hipSuccess ? err : hipMemcpy(p.d_coefs, coefs, (size_t)naccel * sizeof(int64_t), hipMemcpyHostToDevice);
    };
    return open_plan<rtlws_accel_plan>("rtlws_accel_open", why_not_table(log2n, levels, norm, seg, klo, naccel, coefs), e, log2n, levels, norm, seg,
                                       klo, max_trials, upload, rtlws_accel_close);
}

size_t rtlws_accel_workspace_bytes(const rtlws_accel_plan* p) { return p ? p->ws_bytes : 0; }

int rtlws_accel_search(rtlws_accel_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best, int32_t* d_at,
                       float* d_power, float* d_white, void* stream)
{
    const char* fn = "rtlws_accel_search";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_run(ntrials, nsamp, pl::MAX_LOG2N, WHY_LONG_NSAMP, in_stride, d_in, d_best, d_at, d_power, d_white)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if ((long)ntrials * p->naccel > MAX_VIRTUAL) return fail(fn, WHY_VIRTUAL, -1);
    if (nsamp > (1 << p->log2n)) return fail(fn, "nsamp must be at most the plan's N", -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    Params kp;
    kp.s = run_params(*p, d_in, in_stride, nsamp, d_best, d_at, d_power, d_white);
    kp.coefs = p->d_coefs;
    kp.naccel = p->naccel;
    const hipStream_t st = stream_of(p->engine, stream);
    // the groups are of virtual trials: every one reads the caller's series from its first trial on
    err = for_groups(*p, ntrials * p->naccel, [&](int v0, int g) {
        kp.s.trial0 = v0;
        return launch_group(kp, g, st);
    });
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

int rtlws_accel_resample(rtlws_accel_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, int a_first, int a_count,
                         float* d_out, long out_stride, void* stream)
{
    const char* fn = "rtlws_accel_resample";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_input(ntrials, nsamp, pl::MAX_LOG2N, WHY_LONG_NSAMP, in_stride)) return fail(fn, why, -1);
    if (out_stride < nsamp) return fail(fn, "out_stride must be >= nsamp", -1);
    if (out_stride % 4) return fail(fn, "out_stride must be a multiple of 4", -1);
    if (a_count < 1) return fail(fn, "a_count must be >= 1", -1);
    if (a_first < 0) return fail(fn, "a_first must be >= 0", -1);
    if ((long)a_first + a_count > MAX_NACCEL) return fail(fn, "a_first + a_count must be at most naccel (at most 1024)", -1);
    if (!d_in || !d_out) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_in) & 15u) return fail(fn, "d_in must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(fn, "d_out must be 16-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (a_first + a_count > p->naccel) return fail(fn, "a_first + a_count must be at most naccel", -1);
    if ((long)ntrials * a_count > MAX_VIRTUAL) return fail(fn, "ntrials * a_count must be at most 65536", -1);
    if (nsamp > (1 << p->log2n)) return fail(fn, "nsamp must be at most the plan's N", -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    const ResampleParams rp{d_in, d_out, p->d_coefs, in_stride, out_stride, nsamp, a_first, a_count, ntrials * a_count};
    err = launch_resample(rp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

int64_t rtlws_accel_coef(double accel_m_s2, double tsamp_s)
{
    const char* fn = "rtlws_accel_coef";
    g_err.clear();
    if (!std::isfinite(accel_m_s2) || !std::isfinite(tsamp_s)) return fail(fn, "the arguments must be finite", 0);
    bool beyond = false;
    const int64_t c = scaled(accel_m_s2, tsamp_s, 63, 299792458u, beyond);      // 2^64 / (2 c) = 2^63 / c
    if (beyond) return fail(fn, "the coefficient is beyond +-2^40", 0);
    return c;
}

int64_t rtlws_accel_coef_from_shift(double mid_shift_samples, int nsamp)
{
    const char* fn = "rtlws_accel_coef_from_shift";
    g_err.clear();
    if (!std::isfinite(mid_shift_samples)) return fail(fn, "the shift must be finite", 0);
    if (nsamp < 2 || nsamp > (1 << pl::MAX_LOG2N)) return fail(fn, "nsamp must be 2 .. 4194304", 0);
    bool beyond = false;
    const uint64_t last = (uint64_t)nsamp - 1;
    const int64_t c = scaled(mid_shift_samples, 1.0, 66, last * last, beyond);   // 4 * 2^64 / L^2
    if (beyond) return fail(fn, "the coefficient is beyond +-2^40", 0);
    return c;
}

long rtlws_accel_shift(int64_t coef, int nsamp, int n)
{
    const char* fn = "rtlws_accel_shift";
    g_err.clear();
    if (coef < -MAX_COEF || coef > MAX_COEF) return fail(fn, "the coefficient must be -2^40 .. 2^40", 0);
    if (nsamp < 1 || nsamp > (1 << pl::MAX_LOG2N)) return fail(fn, WHY_LONG_NSAMP, 0);
    if (n < 0 || n >= nsamp) return fail(fn, "n must be 0 .. nsamp - 1", 0);
    return shift(coef, n, nsamp - 1);
}

}  // extern "C"

// period_shim.hip -- extern "C" glue of include/rtlws_period.h (librtlws_period.so): argument rules, the plan and its
// table, the launch, and the host's helpers (the period of a bin, the false-alarm probability of a harmonic sum).  The
// engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on
// the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <limits>
#include <vector>

#include "period.h"
#include "period_plan.h"
#include "rtlws_period.h"
#include "twiddle_tables.h"

// The transform's table on the engine's device
struct rtlws_period_plan {
    rtlws_engine* engine;
    int device;
    int log2n, levels, log2norm, seg, klo;
    float2* d_tw;              // [N / 2] e^(-2 pi i j / N)
};

namespace {

using namespace rtlws::period;

static_assert(MIN_LOG2N == RTLWS_PERIOD_MIN_LOG2N && MAX_LOG2N == RTLWS_PERIOD_MAX_LOG2N && MAX_LEVELS == RTLWS_PERIOD_MAX_LEVELS &&
                  MIN_NORM == RTLWS_PERIOD_MIN_NORM && MIN_SEG == RTLWS_PERIOD_MIN_SEG && MAX_TRIALS == RTLWS_PERIOD_MAX_TRIALS,
              "rtlws_period.h and period.h disagree");

// ---- the library's own rules; a run's, ntrials' and the period of a bin are the family's (period_plan.h) ----
const char* why_not_log2n(int log2n) { return log2n < MIN_LOG2N || log2n > MAX_LOG2N ? "log2n must be 10 .. 15" : nullptr; }

const char* why_not_plan(int log2n, int levels, int norm, int seg, int klo)
{
    if (const char* why = why_not_log2n(log2n)) return why;
    const int m = 1 << (log2n - 1);
    if (levels < 1 || levels > MAX_LEVELS) return "levels must be 1 .. 5";
    if (norm < MIN_NORM || norm > m || !power_of_two(norm)) return "norm must be a power of two 16 .. N / 2";
    if (seg < MIN_SEG || seg > m || !power_of_two(seg)) return "seg must be a power of two 64 .. N / 2";
    if (klo < 1 || klo > m - 1) return "klo must be 1 .. N / 2 - 1";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_period_last_error(void) { return g_err.c_str(); }

int rtlws_period_supported(int log2n, int levels, int norm, int seg, int klo)
{
    return supported("rtlws_period", why_not_plan(log2n, levels, norm, seg, klo));
}

int rtlws_period_geometry(int log2n, int levels, int norm, int seg, int klo, int ntrials, int* blocks, int* threads, int* lds, int* nseg)
{
    const char* fn = "rtlws_period_geometry";
    g_err.clear();
    if (const char* why = why_not_plan(log2n, levels, norm, seg, klo)) return fail(fn, why, -1);
    if (const char* why = why_not_ntrials(ntrials)) return fail(fn, why, -1);
    if (blocks) *blocks = ntrials;
    if (threads) *threads = threads_of(log2n);
    if (lds) *lds = lds_bytes(log2n);
    if (nseg) *nseg = (1 << (log2n - 1)) / seg;
    return 0;
}

rtlws_period_plan* rtlws_period_open(rtlws_engine* e, int log2n, int levels, int norm, int seg, int klo)
{
    const char* fn = "rtlws_period_open";
    g_err.clear();
    const int device = open_device(fn, why_not_plan(log2n, levels, norm, seg, klo), e);
    if (device < 0) return nullptr;
    // e^(-2 pi i j / N), j < N / 2: the f64 table of the spectrum kernels (long double, the axis values exact), rounded
    // once more to f32
    const int n = 1 << log2n, m = n / 2;
    const std::vector<rtlws::D2> tw64 = rtlws::tables_f64(n).tw64;
    std::vector<float2> tw((size_t)m);
    for (int j = 0; j < m; ++j) tw[j] = make_float2((float)tw64[j].x, (float)tw64[j].y);
    float2* d_tw = nullptr;
    hipError_t err = hipMalloc(reinterpret_cast<void**>(&d_tw), (size_t)m * sizeof(float2));
    if (err == hipSuccess) err = hipMemcpy(d_tw, tw.data(), (size_t)m * sizeof(float2), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = prepare_period(log2n, device);
    if (err != hipSuccess) {
        if (d_tw) (void)hipFree(d_tw);
        fail_hip(fn, "the table or the kernel", err);
        return nullptr;
    }
    return new rtlws_period_plan{e, device, log2n, levels, log2_of(norm), seg, klo, d_tw};
}

void rtlws_period_close(rtlws_period_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_tw);
    delete p;
}

int rtlws_period_run(rtlws_period_plan* p, const float* d_in, long in_stride, int ntrials, int nsamp, float* d_best, int32_t* d_at,
                     float* d_power, float* d_white, void* stream)
{
    const char* fn = "rtlws_period_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_run(ntrials, nsamp, MAX_LOG2N, "nsamp must be 1 .. 32768", in_stride, d_in, d_best, d_at, d_power, d_white)) return fail(fn, why, -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    if (nsamp > (1 << p->log2n)) return fail(fn, "nsamp must be at most the plan's N", -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    Params kp;
    kp.in = d_in;
    kp.best = d_best;
    kp.at = d_at;
    kp.power = d_power;
    kp.white = d_white;
    kp.tw = p->d_tw;
    kp.in_stride = in_stride;
    kp.nsamp = nsamp;
    kp.levels = p->levels;
    kp.log2norm = p->log2norm;
    kp.seg = p->seg;
    kp.klo = p->klo;
    kp.norm_scale = std::ldexp(1.0f, -p->log2norm);
    err = launch_period(p->log2n, kp, ntrials, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

double rtlws_period_samples(int log2n, int level, int k) { return samples("rtlws_period_samples", why_not_log2n(log2n), log2n, level, k); }

double rtlws_period_lnq(double S, int H)
{
    if (H < 1 || H > 16 || !std::isfinite(S)) return std::numeric_limits<double>::quiet_NaN();
    if (S <= 0.0) return 0.0;
    // ln sum_{j<H} exp(j ln S - ln j!) through its largest term
    const double ls = std::log(S);
    double term[16], top = -std::numeric_limits<double>::infinity();
    for (int j = 0; j < H; ++j) {
        term[j] = (double)j * ls - std::lgamma((double)j + 1.0);
        if (term[j] > top) top = term[j];
    }
    double sum = 0.0;
    for (int j = 0; j < H; ++j) sum += std::exp(term[j] - top);
    const double lnq = -S + top + std::log(sum);
    return lnq < 0.0 ? lnq : 0.0;                              // a probability: the sum's rounding may not lift it above 1
}

}  // extern "C"

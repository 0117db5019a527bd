// cdd_shim.hip -- extern "C" glue of include/rtlws_cdd.h (librtlws_cdd.so): argument rules, the plan with its tables (the
// channels' filters in the order of the kernel's places, the transform's twiddles), the launch of a run, and the host's
// helpers (the chirp of a channel, the overlap it needs).  The engine (device, stream) is librtlws_hip.so's; nothing here
// reads the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "cdd.h"
#include "rtlws_cdd.h"
#include "search_plan.h"

struct rtlws_cdd_plan : rtlws::search::Plan {
    int log2n, lead, trail, hop, nchan, ksum;
    float2* d_tables;          // the filters [nchan][N] in the order of the places, then the twiddles [N]
};

namespace {

using namespace rtlws::cdd;
namespace sp = rtlws::search;

static_assert(MIN_LOG2N == RTLWS_CDD_MIN_LOG2_NFFT && MAX_LOG2N == RTLWS_CDD_MAX_LOG2_NFFT && MAX_NCHAN == RTLWS_CDD_MAX_NCHAN &&
                  MAX_NSEG == RTLWS_CDD_MAX_NSEG && CHANNEL_MAJOR == RTLWS_CDD_CHANNEL_MAJOR && TIME_MAJOR == RTLWS_CDD_TIME_MAJOR,
              "rtlws_cdd.h and cdd.h disagree");

constexpr double DISPERSION = sp::DISPERSION * 1e6;           // the band's constant, in microseconds MHz^2
constexpr double TWO_PI = 6.283185307179586476925286766559;

// ---- the rules, each worded once ----
const char* why_not_log2(int log2_nfft) { return log2_nfft < MIN_LOG2N || log2_nfft > MAX_LOG2N ? "log2_nfft must be 9 .. 14" : nullptr; }

const char* why_not_plan(int log2_nfft, int lead, int trail, int nchan, int ksum)
{
    if (const char* why = why_not_log2(log2_nfft)) return why;
    if (lead < 0 || trail < 0) return "lead and trail must be >= 0";
    const long hop = (1L << log2_nfft) - lead - trail;
    if (hop < 1) return "hop = N - lead - trail must be >= 1";
    if (nchan < 1 || nchan > MAX_NCHAN) return "nchan must be 1 .. 1024";
    if (ksum < 0 || ksum > hop) return "ksum must be 0 .. hop";
    if (ksum && hop % ksum) return "ksum must divide hop";
    return nullptr;
}

const char* why_not_nseg(long nseg) { return nseg < 0 || nseg > MAX_NSEG ? "nseg must be 0 .. 1048576" : nullptr; }

const char* why_not_band(double f0, double rate, double dm)
{
    if (!std::isfinite(f0) || !std::isfinite(rate) || !std::isfinite(dm)) return "the arguments must be finite";
    if (rate == 0.0) return "rate_mhz must not be 0";
    if (!(f0 - std::fabs(rate) / 2 > 0.0)) return "the band's lower edge f_centre - |rate| / 2 must be > 0";
    if (dm < 0.0) return "dm must be >= 0";
    return nullptr;
}

long needed(const rtlws_cdd_plan& p, long nseg) { return nseg ? (nseg - 1) * p.hop + (1L << p.log2n) : 0; }

}  // namespace

extern "C" {

const char* rtlws_cdd_last_error(void) { return g_err.c_str(); }

int rtlws_cdd_supported(int log2_nfft, int lead, int trail, int nchan, int ksum)
{
    return supported("rtlws_cdd", why_not_plan(log2_nfft, lead, trail, nchan, ksum));
}

int rtlws_cdd_geometry(int log2_nfft, int lead, int trail, int nchan, int ksum, long nseg, int* blocks, int* threads, int* lds_bytes)
{
    const char* fn = "rtlws_cdd_geometry";
    g_err.clear();
    if (const char* why = why_not_plan(log2_nfft, lead, trail, nchan, ksum)) return fail(fn, why, -1);
    if (const char* why = why_not_nseg(nseg)) return fail(fn, why, -1);
    if (blocks) *blocks = (int)(nseg * nchan);
    if (threads) *threads = threads_of(log2_nfft);
    if (lds_bytes) *lds_bytes = lds_of(log2_nfft);
    return 0;
}

rtlws_cdd_plan* rtlws_cdd_open(rtlws_engine* e, int log2_nfft, int lead, int trail, int nchan, int ksum, const float* tables)
{
    const char* why = why_not_plan(log2_nfft, lead, trail, nchan, ksum);
    if (!why && !tables) why = "null tables";
    const auto fill = [&](rtlws_cdd_plan& p) {
        const int n = 1 << log2_nfft;
        p.log2n = log2_nfft, p.lead = lead, p.trail = trail, p.hop = n - lead - trail, p.nchan = nchan, p.ksum = ksum;
        // bin k of a channel goes where forward leaves it; behind the filters e^(-2 pi i j / (2 N)), j < N, rounded once
        std::vector<float2> host((size_t)(nchan + 1) * n);
        for (int c = 0; c < nchan; ++c)
            for (int k = 0; k < n; ++k) {
                const float* const h = tables + 2 * ((size_t)c * n + k);
                host[(size_t)c * n + pos_of(log2_nfft, k)] = make_float2(h[0], h[1]);
            }
        const long double step = 3.141592653589793238462643383279L / (long double)n;
        for (int j = 0; j < n; ++j) host[(size_t)nchan * n + j] = make_float2((float)cosl(step * j), (float)-sinl(step * j));
        const hipError_t err = sp::upload(&p.d_tables, host.data(), host.size());
        return err == hipSuccess ? prepare(log2_nfft, p.device) : err;
    };
    return sp::open_plan<rtlws_cdd_plan>("rtlws_cdd_open", why, e, fill, "the tables or the kernel", rtlws_cdd_close);
}

void rtlws_cdd_close(rtlws_cdd_plan* p) { sp::close_plan(p, &rtlws_cdd_plan::d_tables); }

long rtlws_cdd_samples_needed(const rtlws_cdd_plan* p, long nseg)
{
    const char* fn = "rtlws_cdd_samples_needed";
    g_err.clear();
    if (!p) return fail(fn, NULL_PLAN, -1);
    if (nseg < 0) return fail(fn, "nseg must be >= 0", -1);
    return needed(*p, nseg);
}

int rtlws_cdd_run(rtlws_cdd_plan* p, const float* d_in, long in_stride, long nseg, float* d_out, long out_stride, int layout, void* stream)
{
    const char* fn = "rtlws_cdd_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_nseg(nseg)) return fail(fn, why, -1);
    if (layout != CHANNEL_MAJOR && layout != TIME_MAJOR) return fail(fn, "unknown layout", -1);
    if (!d_in || !d_out) return fail(fn, "null pointer", -1);
    if (sp::misaligned(d_in, 8)) return fail(fn, "d_in must be 8-byte aligned", -1);
    if (sp::misaligned(d_out, 4)) return fail(fn, "d_out must be 4-byte aligned", -1);
    if (!p) return fail(fn, NULL_PLAN, -1);
    // what the plan decides; still before anything is asked of the device
    const long rows = p->ksum ? nseg * (p->hop / p->ksum) : nseg * p->hop;        // of a channel
    if (!p->ksum && layout != CHANNEL_MAJOR) return fail(fn, "voltages are channel-major", -1);
    if (!p->ksum && sp::misaligned(d_out, 8)) return fail(fn, "d_out must be 8-byte aligned for voltages", -1);
    if (in_stride < needed(*p, nseg)) return fail(fn, "in_stride must be >= samples_needed", -1);
    if (layout == TIME_MAJOR ? out_stride < p->nchan : out_stride < rows)
        return fail(fn, layout == TIME_MAJOR ? "out_stride must be >= nchan" : "out_stride must be >= the outputs of a channel", -1);
    if (nseg == 0) return 0;

    if (sp::use_device(fn, p)) return -3;
    Params kp{};
    kp.in = reinterpret_cast<const float2*>(d_in);
    kp.out = d_out;
    kp.table = p->d_tables;
    kp.tw = p->d_tables + ((size_t)p->nchan << p->log2n);
    kp.in_stride = in_stride, kp.out_stride = out_stride;
    kp.lead = p->lead, kp.hop = p->hop, kp.ksum = p->ksum, kp.layout = layout;
    kp.scale = 1.0f / (float)(1 << p->log2n);
    const hipError_t err = launch(p->log2n, kp, nseg, p->nchan, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

int rtlws_cdd_chirp(int log2_nfft, double f_centre_mhz, double rate_mhz, double dm, float* re_im)
{
    const char* fn = "rtlws_cdd_chirp";
    g_err.clear();
    if (const char* why = why_not_log2(log2_nfft)) return fail(fn, why, -1);
    if (!re_im) return fail(fn, "null table", -1);
    if (const char* why = why_not_band(f_centre_mhz, rate_mhz, dm)) return fail(fn, why, -1);
    const int n = 1 << log2_nfft;
    const double f0 = f_centre_mhz;
    for (int k = 0; k < n; ++k) {
        const double f = (double)(k < n / 2 ? k : k - n) * rate_mhz / (double)n;
        double phi = DISPERSION * dm * f * f / (f0 * f0 * (f0 + f));
        phi -= std::rint(phi);
        re_im[2 * k] = (float)std::cos(TWO_PI * phi);
        re_im[2 * k + 1] = (float)-std::sin(TWO_PI * phi);
    }
    return 0;
}

int rtlws_cdd_overlap(double f_centre_mhz, double rate_mhz, double dm, int* lead, int* trail)
{
    const char* fn = "rtlws_cdd_overlap";
    g_err.clear();
    if (!lead || !trail) return fail(fn, "null pointer", -1);
    if (const char* why = why_not_band(f_centre_mhz, rate_mhz, dm)) return fail(fn, why, -1);
    const double f0 = f_centre_mhz, w = std::fabs(rate_mhz), half = w / 2;
    const auto tau = [&](double f) { return DISPERSION * dm * (1.0 / ((f0 + f) * (f0 + f)) - 1.0 / (f0 * f0)) * w; };
    const double late = std::ceil(tau(-half)), early = std::ceil(-tau(half));
    if (late > 1073741824.0 || early > 1073741824.0) return fail(fn, "a delay above 2^30 samples", -1);
    *trail = (int)late, *lead = (int)early;
    return 0;
}

}  // extern "C"

// ddcfir_shim.hip -- extern "C" glue of include/rtlws_ddcfir.h (librtlws_ddcfir.so): the filter design, the taps on
// the device, argument rules, geometry, the launch.  The plan's base (the phasor table on the device), its open and
// close and the rules it shares with the other tuned-channel libraries are ddc_plan.h's; decim and
// ntaps keep its own words.  The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment,
// and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "ddc_plan.h"
#include "ddcfir.h"
#include "rtlws_ddc.h"
#include "rtlws_ddcfir.h"

struct rtlws_ddcfir_plan : rtlws::ddc::Plan {
    int decim, ntaps;
    int16_t* d_taps;
};

namespace {

using namespace rtlws::ddcfir;
namespace ddc = rtlws::ddc;

static_assert(rtlws::ddc::LOG2_P == RTLWS_DDC_LOG2_PERIOD && MAX_CH == RTLWS_DDCFIR_MAX_CHANNELS && MAX_R == RTLWS_DDCFIR_MAX_DECIM &&
                  MAX_TAPS == RTLWS_DDCFIR_MAX_TAPS && MAX_TAP == RTLWS_DDCFIR_MAX_TAP && MAX_SHIFT == RTLWS_DDCFIR_MAX_SHIFT,
              "rtlws_ddcfir.h, rtlws_ddc.h and ddcfir.h disagree");
static_assert(lds_bytes(MAX_TAPS, MAX_CH) == 64 * 1024, "the operands of the largest launch: 64 KiB");

// the filter's shape, or nullptr
const char* why_not_filter(int decim, int ntaps)
{
    if (decim < 1 || decim > MAX_R) return "decim must be 1 .. 128";
    if (ntaps < 1 || ntaps > MAX_TAPS) return "ntaps must be 1 .. 256";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_ddcfir_last_error(void) { return g_err.c_str(); }

int rtlws_ddcfir_supported(int decim, int ntaps, int nchannels)
{
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = ddc::why_not_channels(nchannels);
    return supported("rtlws_ddcfir", why);
}

long rtlws_ddcfir_samples_needed(int decim, int ntaps, long dec_len)
{
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = ddc::why_not_dec_len(dec_len);
    if (why) return fail("rtlws_ddcfir_samples_needed", why, -1);
    return dec_len == 0 ? 0 : (dec_len - 1) * decim + ntaps;
}

int rtlws_ddcfir_grid(int decim, int ntaps, int nchannels, long dec_len, int* blocks, int* threads, int* lds_bytes_out,
                      int* tile_dec)
{
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = ddc::why_not_channels(nchannels);
    if (!why) why = ddc::why_not_dec_len(dec_len);
    if (why) return fail("rtlws_ddcfir_grid", why, -1);
    if (blocks) *blocks = (int)ddc::tiles_of(dec_len);
    if (threads) *threads = THREADS;
    if (lds_bytes_out) *lds_bytes_out = lds_bytes(ntaps, nchannels);
    if (tile_dec) *tile_dec = TILE_DEC;
    return 0;
}

int rtlws_ddcfir_design(int decim, int ntaps, int16_t* taps)
{
    g_err.clear();
    if (const char* why = why_not_filter(decim, ntaps)) return fail("rtlws_ddcfir_design", why, -1);
    if (!taps) return fail("rtlws_ddcfir_design", "null pointer", -1);
    std::vector<double> p((size_t)ntaps);
    double sum = 0.0, peak = 0.0;
    for (int n = 0; n < ntaps; ++n) {
        const double x = ((double)n - (double)(ntaps - 1) / 2.0) / (double)decim;
        const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double w = ntaps == 1 ? 1.0 : 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)n / (double)(ntaps - 1));
        p[n] = sinc * w;
        sum += p[n];
        peak = std::fmax(peak, std::fabs(p[n]));
    }
    const double a = std::fmin(16384.0 * (double)decim / sum, (double)MAX_TAP / peak);
    for (int n = 0; n < ntaps; ++n) taps[n] = (int16_t)std::rint(a * p[n]);
    return 0;
}

int rtlws_ddcfir_bound(int ntaps, const int16_t* taps, int out_shift, double* bound)
{
    g_err.clear();
    if (const char* why = why_not_filter(1, ntaps)) return fail("rtlws_ddcfir_bound", why, -1);
    if (out_shift < 0 || out_shift > MAX_SHIFT) return fail("rtlws_ddcfir_bound", "out_shift must be 0 .. 30", -1);
    if (!taps || !bound) return fail("rtlws_ddcfir_bound", "null pointer", -1);
    double sum = 0.0;
    for (int n = 0; n < ntaps; ++n) sum += std::fabs((double)taps[n]);
    *bound = 0.5 + std::sqrt(2.0) * (sum / 128.0 + 128.0 * ntaps + 182.0 * (sum + ntaps) / 32768.0) / std::ldexp(1.0, out_shift);
    return 0;
}

rtlws_ddcfir_plan* rtlws_ddcfir_open(rtlws_engine* e, int decim, int ntaps, const int16_t* taps)
{
    const char* fn = "rtlws_ddcfir_open";
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why && !taps) why = "null taps";
    if (!why)
        for (int n = 0; n < ntaps; ++n)
            if (taps[n] < -MAX_TAP || taps[n] > MAX_TAP)
                why = "a tap lies outside [-32639, 32639] (the filter is applied as two int8 operands, 256 * high + low: beyond "
                      "the limit the high one leaves int8)";
    const size_t bytes = (size_t)ntaps * sizeof(int16_t);
    return ddc::open_plan<rtlws_ddcfir_plan>(
        fn, why, e,
        [&](rtlws_ddcfir_plan& p) {
            p.decim = decim;
            p.ntaps = ntaps;
            hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.d_taps), bytes);
            if (err == hipSuccess) err = hipMemcpy(p.d_taps, taps, bytes, hipMemcpyHostToDevice);
            if (err == hipSuccess) err = prepare_bank(decim, ntaps, p.device);
            if (err != hipSuccess) (void)hipFree(p.d_taps);
            return err;
        },
        "the taps, the table or the kernel");
}

void rtlws_ddcfir_close(rtlws_ddcfir_plan* p)
{
    if (p && hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_taps);
    ddc::close_plan(p);
}

int rtlws_ddcfir_run(rtlws_ddcfir_plan* p, const void* d_iq_cu8, long dec_len, long first_dec_index, int nchannels,
                     const int* tuning_words, int out_shift, void* d_out_cs32, long out_stride, void* stream)
{
    const char* fn = "rtlws_ddcfir_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = ddc::why_not_channels(nchannels)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_dec_len(dec_len)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_first(first_dec_index)) return fail(fn, why, -1);
    if (out_shift < 0 || out_shift > MAX_SHIFT) return fail(fn, "out_shift must be 0 .. 30", -1);
    if (const char* why = ddc::why_not_out_stride(out_stride, dec_len)) return fail(fn, why, -1);
    FirParams fp;
    if (const char* why = ddc::fill_words(fp.words, tuning_words, nchannels)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_capture(dec_len > 0, d_iq_cu8, d_out_cs32)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_cs32(d_out_cs32)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_plan(p)) return fail(fn, why, -1);
    // the plan's shape decides nothing further: every (decim, ntaps) a plan holds serves every count above
    if (dec_len == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    fp.src = d_iq_cu8;
    fp.out = d_out_cs32;
    fp.table = p->d_table;
    fp.taps = p->d_taps;
    fp.dec_len = dec_len;
    fp.first = first_dec_index;
    fp.out_stride = out_stride;
    fp.decim = p->decim;
    fp.ntaps = p->ntaps;
    fp.nch = nchannels;
    fp.shift = out_shift;
    err = launch_bank(fp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

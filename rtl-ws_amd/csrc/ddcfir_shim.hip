// ddcfir_shim.hip -- extern "C" glue of include/rtlws_ddcfir.h (librtlws_ddcfir.so): the filter design, the taps and
// the phasor table on the device, argument rules, geometry, the launch.  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ddc_table.h"
#include "ddcfir.h"
#include "rtlws_ddc.h"
#include "rtlws_ddcfir.h"
#include "shim_common.h"

struct rtlws_ddcfir_plan {
    rtlws_engine* engine;
    int device;
    int decim, ntaps;
    uint32_t* d_table;
    int16_t* d_taps;
};

namespace {

using namespace rtlws::ddcfir;

static_assert(rtlws::ddc::LOG2_P == RTLWS_DDC_LOG2_PERIOD && MAX_CH == RTLWS_DDCFIR_MAX_CHANNELS && MAX_R == RTLWS_DDCFIR_MAX_DECIM &&
                  MAX_TAPS == RTLWS_DDCFIR_MAX_TAPS && MAX_TAP == RTLWS_DDCFIR_MAX_TAP && MAX_SHIFT == RTLWS_DDCFIR_MAX_SHIFT,
              "rtlws_ddcfir.h, rtlws_ddc.h and ddcfir.h disagree");
static_assert(lds_bytes(MAX_TAPS, MAX_CH) == 64 * 1024, "the operands of the largest launch: 64 KiB");

long tiles_of(long dec_len) { return (dec_len + TILE_DEC - 1) / TILE_DEC; }

// the rules, each stated once and returning its text or nullptr
const char* why_not_filter(int decim, int ntaps)
{
    if (decim < 1 || decim > MAX_R) return "decim must be 1 .. 128";
    if (ntaps < 1 || ntaps > MAX_TAPS) return "ntaps must be 1 .. 256";
    return nullptr;
}

const char* why_not_channels(int nchannels) { return nchannels < 1 || nchannels > MAX_CH ? "nchannels must be 1 .. 32" : nullptr; }

const char* why_not_count(long dec_len)
{
    if (dec_len < 0) return "dec_len must be >= 0";
    if (dec_len > (long)INT_MAX * TILE_DEC) return "more decimated samples than one grid holds";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_ddcfir_last_error(void) { return g_err.c_str(); }

int rtlws_ddcfir_supported(int decim, int ntaps, int nchannels)
{
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = why_not_channels(nchannels);
    if (why) fail("rtlws_ddcfir", why, 0);
    return why ? 0 : 1;
}

long rtlws_ddcfir_samples_needed(int decim, int ntaps, long dec_len)
{
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = why_not_count(dec_len);
    if (why) return fail("rtlws_ddcfir_samples_needed", why, -1);
    return dec_len == 0 ? 0 : (dec_len - 1) * decim + ntaps;
}

int rtlws_ddcfir_grid(int decim, int ntaps, int nchannels, long dec_len, int* blocks, int* threads, int* lds_bytes_out,
                      int* tile_dec)
{
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why) why = why_not_channels(nchannels);
    if (!why) why = why_not_count(dec_len);
    if (why) return fail("rtlws_ddcfir_grid", why, -1);
    if (blocks) *blocks = (int)tiles_of(dec_len);
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
    if (!why && !e) why = "null engine (no usable HIP device: there is no CPU path)";
    if (why) {
        fail(fn, why, -1);
        return nullptr;
    }
    const int device = rtlws_engine_device(e);
    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        fail_hip(fn, "hipSetDevice", err);
        return nullptr;
    }
    std::vector<int16_t> host(2 * (size_t)P);
    rtlws::ddc::build_table(host.data(), P);
    uint32_t* d_table = nullptr;
    int16_t* d_taps = nullptr;
    err = hipMalloc(reinterpret_cast<void**>(&d_table), host.size() * sizeof(int16_t));
    if (err == hipSuccess) err = hipMalloc(reinterpret_cast<void**>(&d_taps), (size_t)ntaps * sizeof(int16_t));
    if (err == hipSuccess) err = hipMemcpy(d_table, host.data(), host.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = hipMemcpy(d_taps, taps, (size_t)ntaps * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = prepare_bank(decim, ntaps, device);
    if (err != hipSuccess) {
        fail_hip(fn, "the taps, the table or the kernel", err);
        if (d_table) (void)hipFree(d_table);
        if (d_taps) (void)hipFree(d_taps);
        return nullptr;
    }
    return new rtlws_ddcfir_plan{e, device, decim, ntaps, d_table, d_taps};
}

void rtlws_ddcfir_close(rtlws_ddcfir_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) {
        (void)hipFree(p->d_table);
        (void)hipFree(p->d_taps);
    }
    delete p;
}

int rtlws_ddcfir_run(rtlws_ddcfir_plan* p, const void* d_iq_cu8, long dec_len, long first_dec_index, int nchannels,
                     const int* tuning_words, int out_shift, void* d_out_cs32, long out_stride, void* stream)
{
    const char* fn = "rtlws_ddcfir_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_channels(nchannels)) return fail(fn, why, -1);
    if (const char* why = why_not_count(dec_len)) return fail(fn, why, -1);
    if (first_dec_index < 0) return fail(fn, "first_dec_index must be >= 0", -1);
    if (out_shift < 0 || out_shift > MAX_SHIFT) return fail(fn, "out_shift must be 0 .. 30", -1);
    if (out_stride < dec_len) return fail(fn, "out_stride must be >= dec_len", -1);
    if (!tuning_words) return fail(fn, "null tuning_words", -1);
    FirParams fp;
    for (int c = 0; c < MAX_CH; ++c) {
        const int k = c < nchannels ? tuning_words[c] : 0;
        if (k < -P / 2 || k >= P / 2) return fail(fn, "a tuning word lies outside [-32768, 32768)", -1);
        fp.words[c] = (int16_t)k;
    }
    if (dec_len > 0 && (!d_iq_cu8 || !d_out_cs32)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u) return fail(fn, "d_iq_cu8 must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out_cs32) & 7u) return fail(fn, "d_out_cs32 must be 8-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
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

// ddc_shim.hip -- extern "C" glue of include/rtlws_ddc.h (librtlws_ddc.so): argument rules, geometry, the launch.  The
// plan (the phasor table on the device), its open and close and the rules it shares with the other tuned-channel
// libraries are ddc_plan.h's.  The engine (device, stream) is librtlws_hip.so's; nothing here reads
// the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "ddc_bank.h"
#include "ddc_plan.h"
#include "rtlws_ddc.h"

struct rtlws_ddc_plan : rtlws::ddc::Plan {};

namespace {

using namespace rtlws::ddc;

static_assert(LOG2_P == RTLWS_DDC_LOG2_PERIOD && MAX_CH == RTLWS_DDC_MAX_CHANNELS, "rtlws_ddc.h and ddc_bank.h disagree");

// why a shape is not served, or nullptr
const char* why_not(int cic_r, int nchannels, long dec_len)
{
    if (const char* why = why_not_cic_r(cic_r)) return why;
    if (const char* why = why_not_channels(nchannels)) return why;
    return why_not_dec_len(dec_len);
}

}  // namespace

extern "C" {

const char* rtlws_ddc_last_error(void) { return g_err.c_str(); }

int rtlws_ddc_supported(int cic_r, int nchannels)
{
    return supported("rtlws_ddc", why_not(cic_r, nchannels, 0));
}

int rtlws_ddc_table(int16_t* cos_sin)
{
    g_err.clear();
    if (!cos_sin) return fail("rtlws_ddc_table", "null pointer", -1);
    build_table(cos_sin, P);
    return 0;
}

int rtlws_ddc_tuning_word(double offset_hz, double sample_rate_hz, int* word)
{
    g_err.clear();
    if (!word) return fail("rtlws_ddc_tuning_word", "null pointer", -1);
    if (!std::isfinite(offset_hz) || !std::isfinite(sample_rate_hz)) return fail("rtlws_ddc_tuning_word", "non-finite argument", -1);
    if (sample_rate_hz <= 0) return fail("rtlws_ddc_tuning_word", "sample_rate_hz must be > 0", -1);
    const double turns = offset_hz / sample_rate_hz;
    if (!std::isfinite(turns * P)) return fail("rtlws_ddc_tuning_word", "non-finite argument", -1);
    double w = std::fmod(std::rint(turns * P), (double)P);              // (-P, P), exact
    if (w >= P / 2) w -= P;
    if (w < -P / 2) w += P;
    *word = (int)w;
    return 0;
}

int rtlws_ddc_grid(int cic_r, int nchannels, long dec_len, int* blocks, int* threads, int* lds_bytes, int* tile_dec)
{
    g_err.clear();
    if (const char* why = why_not(cic_r, nchannels, dec_len)) return fail("rtlws_ddc_grid", why, -1);
    const bool in_regs = rt_of(cic_r) != 0;                             // the phasor operands: registers or LDS
    if (blocks) *blocks = (int)tiles_of(dec_len);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = in_regs ? 0 : LDS_BYTES_ANY;
    if (tile_dec) *tile_dec = TILE_DEC;
    return 0;
}

rtlws_ddc_plan* rtlws_ddc_open(rtlws_engine* e)
{
    g_err.clear();
    return open_plan<rtlws_ddc_plan>("rtlws_ddc_open", nullptr, e, [](Plan&) { return prepare_bank(); });
}

void rtlws_ddc_close(rtlws_ddc_plan* p) { close_plan(p); }

int rtlws_ddc_run(rtlws_ddc_plan* p, int cic_r, const void* d_iq_cu8, long dec_len, long first_dec_index,
                  int nchannels, const int* tuning_words, void* d_out_cs32, long out_stride, void* stream)
{
    const char* fn = "rtlws_ddc_run";
    g_err.clear();
    if (const char* why = why_not(cic_r, nchannels, dec_len)) return fail(fn, why, -1);
    if (const char* why = why_not_first(first_dec_index)) return fail(fn, why, -1);
    if (const char* why = why_not_out_stride(out_stride, dec_len)) return fail(fn, why, -1);
    BankParams bp;
    if (const char* why = fill_words(bp.words, tuning_words, nchannels)) return fail(fn, why, -1);
    if (const char* why = why_not_capture(dec_len > 0, d_iq_cu8, d_out_cs32)) return fail(fn, why, -1);
    if (const char* why = why_not_cs32(d_out_cs32)) return fail(fn, why, -1);
    if (const char* why = why_not_plan(p)) return fail(fn, why, -1);
    if (dec_len == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    hipStream_t st = stream_of(p->engine, stream);
    bp.src = d_iq_cu8;
    bp.out = d_out_cs32;
    bp.table = p->d_table;
    bp.dec_len = dec_len;
    bp.first = first_dec_index;
    bp.out_stride = out_stride;
    bp.cic_r = cic_r;
    bp.nch = nchannels;
    err = launch_bank(bp, st);
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

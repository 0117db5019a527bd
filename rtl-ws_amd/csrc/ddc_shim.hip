// ddc_shim.hip -- extern "C" glue of include/rtlws_ddc.h (librtlws_ddc.so): the phasor table, argument rules,
// geometry, the launch.  The engine (device, stream) is librtlws_hip.so's; nothing here reads the environment, and
// nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstdint>
#include <vector>

#include "ddc_bank.h"
#include "ddc_table.h"
#include "rtlws_ddc.h"
#include "shim_common.h"

struct rtlws_ddc_plan {
    rtlws_engine* engine;
    int device;
    uint32_t* d_table;
};

namespace {

using namespace rtlws::ddc;

static_assert(LOG2_P == RTLWS_DDC_LOG2_PERIOD && MAX_CH == RTLWS_DDC_MAX_CHANNELS, "rtlws_ddc.h and ddc_bank.h disagree");

long tiles_of(long dec_len) { return (dec_len + TILE_DEC - 1) / TILE_DEC; }

// why a shape is not served, or nullptr
const char* why_not(int cic_r, int nchannels, long dec_len)
{
    if (cic_r < 1 || cic_r > MAX_R) return "cic_r must be 1 .. 128";
    if (nchannels < 1 || nchannels > MAX_CH) return "nchannels must be 1 .. 32";
    if (dec_len < 0) return "dec_len must be >= 0";
    if (dec_len > (long)INT_MAX * TILE_DEC) return "more decimated samples than one grid holds";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_ddc_last_error(void) { return g_err.c_str(); }

int rtlws_ddc_supported(int cic_r, int nchannels)
{
    g_err.clear();
    const char* why = why_not(cic_r, nchannels, 0);
    if (why) fail("rtlws_ddc", why, 0);
    return why ? 0 : 1;
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
    const bool in_regs = cic_r == 8 || cic_r == 10 || cic_r == 12;      // the phasor operands: registers or LDS
    if (blocks) *blocks = (int)tiles_of(dec_len);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = in_regs ? 0 : LDS_BYTES_ANY;
    if (tile_dec) *tile_dec = TILE_DEC;
    return 0;
}

rtlws_ddc_plan* rtlws_ddc_open(rtlws_engine* e)
{
    g_err.clear();
    if (!e) {
        fail("rtlws_ddc_open", "null engine (no usable HIP device: there is no CPU path)", -1);
        return nullptr;
    }
    const int device = rtlws_engine_device(e);
    hipError_t err = hipSetDevice(device);
    if (err != hipSuccess) {
        fail_hip("rtlws_ddc_open", "hipSetDevice", err);
        return nullptr;
    }
    std::vector<int16_t> host(2 * (size_t)P);
    build_table(host.data(), P);
    uint32_t* d_table = nullptr;
    err = hipMalloc(reinterpret_cast<void**>(&d_table), host.size() * sizeof(int16_t));
    if (err == hipSuccess) err = hipMemcpy(d_table, host.data(), host.size() * sizeof(int16_t), hipMemcpyHostToDevice);
    if (err == hipSuccess) err = prepare_bank();
    if (err != hipSuccess) {
        fail_hip("rtlws_ddc_open", "the table or the kernels", err);
        if (d_table) (void)hipFree(d_table);
        return nullptr;
    }
    return new rtlws_ddc_plan{e, device, d_table};
}

void rtlws_ddc_close(rtlws_ddc_plan* p)
{
    if (!p) return;
    if (hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_table);
    delete p;
}

int rtlws_ddc_run(rtlws_ddc_plan* p, int cic_r, const void* d_iq_cu8, long dec_len, long first_dec_index,
                  int nchannels, const int* tuning_words, void* d_out_cs32, long out_stride, void* stream)
{
    const char* fn = "rtlws_ddc_run";
    g_err.clear();
    if (const char* why = why_not(cic_r, nchannels, dec_len)) return fail(fn, why, -1);
    if (first_dec_index < 0) return fail(fn, "first_dec_index must be >= 0", -1);
    if (out_stride < dec_len) return fail(fn, "out_stride must be >= dec_len", -1);
    if (!tuning_words) return fail(fn, "null tuning_words", -1);
    BankParams bp;
    for (int c = 0; c < MAX_CH; ++c) {
        const int k = c < nchannels ? tuning_words[c] : 0;
        if (k < -P / 2 || k >= P / 2) return fail(fn, "a tuning word lies outside [-32768, 32768)", -1);
        bp.words[c] = (int16_t)k;
    }
    if (dec_len > 0 && (!d_iq_cu8 || !d_out_cs32)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u) return fail(fn, "d_iq_cu8 must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out_cs32) & 7u) return fail(fn, "d_out_cs32 must be 8-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
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

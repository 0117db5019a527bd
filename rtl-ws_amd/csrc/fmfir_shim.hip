// fmfir_shim.hip -- extern "C" glue of include/rtlws_fmfir.h (librtlws_fmfir.so): the taps on the device, argument
// rules, geometry, the launch.  The plan's base (the phasor table on the device), its open and close and the family's
// rules are ddc_plan.h's; the block rules and the filter's rules are spelled here as
// fmbank_shim.hip and ddcfir_shim.hip spell them.  The engine (device, stream) is librtlws_hip.so's; nothing here reads the
// environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ddc_plan.h"
#include "fmfir.h"
#include "rtlws_ddc.h"
#include "rtlws_ddcfir.h"
#include "rtlws_fm.h"
#include "rtlws_fmfir.h"

struct rtlws_fmfir_plan : rtlws::ddc::Plan {
    int decim, ntaps;
    int16_t* d_taps;
};

namespace {

using namespace rtlws::fmfir;
namespace ddc = rtlws::ddc;

static_assert(MAX_CH == RTLWS_FMFIR_MAX_CHANNELS && MAX_CH == RTLWS_DDCFIR_MAX_CHANNELS && STATE == RTLWS_FM_STATE_FLOATS &&
                  ddc::LOG2_P == RTLWS_DDC_LOG2_PERIOD && ddc::MAX_R == RTLWS_DDCFIR_MAX_DECIM && MAX_TAPS == RTLWS_DDCFIR_MAX_TAPS &&
                  MAX_TAP == RTLWS_DDCFIR_MAX_TAP && MAX_SHIFT == RTLWS_DDCFIR_MAX_SHIFT,
              "rtlws_fmfir.h, rtlws_ddcfir.h, rtlws_fm.h and fmfir.h disagree");

// The rules below that ddc_plan.h does not hold are fmbank_shim.hip's block rules and ddcfir_shim.hip's filter rules
// in this unit's own spelling, word for word: shared through a header they changed those libraries' host object code
// (DESIGN.md 4.13c), and the existing libraries stay as they are.

long tiles_of(int block_len, long nblocks)
{
    const long total_audio = nblocks * (long)(block_len / 4);
    return (total_audio + TILE - 1) / TILE;
}

long col_tiles(int nchannels) { return (nchannels + COL_CH - 1) / COL_CH; }

// the filter's shape, or nullptr (ddcfir_shim.hip's words)
const char* why_not_filter(int decim, int ntaps)
{
    if (decim < 1 || decim > ddc::MAX_R) return "decim must be 1 .. 128";
    if (ntaps < 1 || ntaps > MAX_TAPS) return "ntaps must be 1 .. 256";
    return nullptr;
}

// why a call's blocks and channels are not served by any plan, or nullptr (fmbank_shim.hip's words): a decimated
// sample advances by at most 2 * 128 bytes, so the sizes of every served filter fit where these pass
const char* why_not_call(int nchannels, int block_len, long nblocks)
{
    if (block_len < RTLWS_FM_MIN_BLOCK_LEN) return "block_len must be >= 20 (the reference's half-band keeps ten samples of a block)";
    if (nblocks < 0) return "nblocks must be >= 0";
    if (const char* why = ddc::why_not_channels(nchannels)) return why;
    if (nblocks > LONG_MAX / ((long)block_len * 2 * ddc::MAX_R)) return "nblocks * block_len too large";
    if (tiles_of(block_len, nblocks) + 1 > (long)INT_MAX / col_tiles(nchannels)) return "more tiles than one grid holds";
    return nullptr;
}

// why a shape is not served, or nullptr: the filter first, as in rtlws_ddcfir_supported
const char* why_not(int decim, int ntaps, int nchannels, int block_len, long nblocks)
{
    if (const char* why = why_not_filter(decim, ntaps)) return why;
    return why_not_call(nchannels, block_len, nblocks);
}

}  // namespace

extern "C" {

const char* rtlws_fmfir_last_error(void) { return g_err.c_str(); }

int rtlws_fmfir_supported(int decim, int ntaps, int nchannels, int block_len, long nblocks)
{
    return supported("rtlws_fmfir", why_not(decim, ntaps, nchannels, block_len, nblocks));
}

long rtlws_fmfir_samples_needed(int decim, int ntaps, int block_len, long nblocks)
{
    g_err.clear();
    if (const char* why = why_not(decim, ntaps, 1, block_len, nblocks)) return fail("rtlws_fmfir_samples_needed", why, -1);
    return nblocks == 0 ? 0 : (nblocks * block_len - 1) * decim + ntaps;
}

int rtlws_fmfir_grid(int decim, int ntaps, int nchannels, int block_len, long nblocks, int* blocks, int* threads,
                     int* lds_bytes, int* tile_audio)
{
    g_err.clear();
    if (const char* why = why_not(decim, ntaps, nchannels, block_len, nblocks)) return fail("rtlws_fmfir_grid", why, -1);
    const bool copy = nblocks == 0;                      // the state copy: one workgroup, no LDS
    if (blocks) *blocks = copy ? 1 : (int)((tiles_of(block_len, nblocks) + 1) * col_tiles(nchannels));
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = copy ? 0 : LDS_BYTES;
    if (tile_audio) *tile_audio = TILE;
    return 0;
}

rtlws_fmfir_plan* rtlws_fmfir_open(rtlws_engine* e, int decim, int ntaps, const int16_t* taps)
{
    const char* fn = "rtlws_fmfir_open";
    g_err.clear();
    const char* why = why_not_filter(decim, ntaps);
    if (!why && !taps) why = "null taps";
    if (!why)
        for (int n = 0; n < ntaps; ++n)
            if (taps[n] < -MAX_TAP || taps[n] > MAX_TAP)
                why = "a tap lies outside [-32639, 32639] (the filter is applied as two int8 operands, 256 * high + low: beyond "
                      "the limit the high one leaves int8)";
    const size_t bytes = (size_t)ntaps * sizeof(int16_t);
    return ddc::open_plan<rtlws_fmfir_plan>(
        fn, why, e,
        [&](rtlws_fmfir_plan& p) {
            p.decim = decim;
            p.ntaps = ntaps;
            hipError_t err = hipMalloc(reinterpret_cast<void**>(&p.d_taps), bytes);
            if (err == hipSuccess) err = hipMemcpy(p.d_taps, taps, bytes, hipMemcpyHostToDevice);
            if (err == hipSuccess) err = prepare_bank(decim, ntaps);
            if (err != hipSuccess) (void)hipFree(p.d_taps);
            return err;
        },
        "the taps, the table or the kernels");
}

void rtlws_fmfir_close(rtlws_fmfir_plan* p)
{
    if (p && hipSetDevice(p->device) == hipSuccess) (void)hipFree(p->d_taps);
    ddc::close_plan(p);
}

int rtlws_fmfir_run(rtlws_fmfir_plan* p, const void* d_iq_cu8, int block_len, long nblocks, long first_dec_index,
                    int nchannels, const int* tuning_words, int out_shift, const float* d_state_in, float* d_state_out,
                    float* d_audio, long audio_stride, void* stream)
{
    const char* fn = "rtlws_fmfir_run";
    g_err.clear();
    // what needs no plan
    if (const char* why = why_not_call(nchannels, block_len, nblocks)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_first(first_dec_index)) return fail(fn, why, -1);
    if (out_shift < 0 || out_shift > MAX_SHIFT) return fail(fn, "out_shift must be 0 .. 30", -1);
    if (audio_stride < nblocks * (long)(block_len / 4)) return fail(fn, "audio_stride must be >= nblocks * quarter", -1);
    BankParams bp;
    if (const char* why = ddc::fill_words(bp.words, tuning_words, nchannels)) return fail(fn, why, -1);
    if (!d_state_in || !d_state_out) return fail(fn, "null state pointer", -1);
    const uintptr_t si = reinterpret_cast<uintptr_t>(d_state_in), so = reinterpret_cast<uintptr_t>(d_state_out);
    const uintptr_t state_bytes = (uintptr_t)nchannels * STATE * sizeof(float);
    if (si < so + state_bytes && so < si + state_bytes) return fail(fn, "d_state_in and d_state_out must not overlap", -1);
    if (const char* why = ddc::why_not_capture(nblocks > 0, d_iq_cu8, d_audio)) return fail(fn, why, -1);
    if ((si | so | reinterpret_cast<uintptr_t>(d_audio)) & 3u)
        return fail(fn, "d_state_in, d_state_out and d_audio must be 4-byte aligned", -1);
    if (const char* why = ddc::why_not_plan(p)) return fail(fn, why, -1);
    // the plan's shape decides nothing further: every (decim, ntaps) a plan holds serves every call above

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    hipStream_t st = stream_of(p->engine, stream);
    if (nblocks == 0) {
        err = launch_state_copy(d_state_in, d_state_out, nchannels * STATE, st);
    } else {
        bp.src = d_iq_cu8;
        bp.table = p->d_table;
        bp.taps = p->d_taps;
        bp.state_in = d_state_in;
        bp.state_out = d_state_out;
        bp.audio = d_audio;
        bp.audio_stride = audio_stride;
        bp.first = first_dec_index;
        bp.nblocks = nblocks;
        bp.ntiles = tiles_of(block_len, nblocks);
        bp.block_len = block_len;
        bp.decim = p->decim;
        bp.ntaps = p->ntaps;
        bp.nch = nchannels;
        bp.shift = out_shift;
        err = launch_bank(bp, st);
    }
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

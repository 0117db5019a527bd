// fmbank_shim.hip -- extern "C" glue of include/rtlws_fmbank.h (librtlws_fmbank.so): argument rules, geometry, the
// launch.  The plan (the phasor table on the device), its open and close and the rules it shares with the other
// tuned-channel libraries are ddc_plan.h's; the block rules are its own.  The engine (device,
// stream) is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host:
// without a device there is no plan.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "ddc_plan.h"
#include "fm_bank.h"
#include "rtlws_ddc.h"
#include "rtlws_fm.h"
#include "rtlws_fmbank.h"

struct rtlws_fmbank_plan : rtlws::ddc::Plan {};

namespace {

using namespace rtlws::fmbank;
namespace ddc = rtlws::ddc;

static_assert(MAX_CH == RTLWS_FMBANK_MAX_CHANNELS && MAX_CH == RTLWS_DDC_MAX_CHANNELS && STATE == RTLWS_FM_STATE_FLOATS &&
                  ddc::LOG2_P == RTLWS_DDC_LOG2_PERIOD,
              "rtlws_fmbank.h, rtlws_ddc.h, rtlws_fm.h and fm_bank.h disagree");

long tiles_of(int block_len, long nblocks)
{
    const long total_audio = nblocks * (long)(block_len / 4);
    return (total_audio + TILE - 1) / TILE;
}

long col_tiles(int nchannels) { return (nchannels + COL_CH - 1) / COL_CH; }

// why a shape is not served, or nullptr
const char* why_not(int cic_r, int nchannels, int block_len, long nblocks)
{
    if (block_len < RTLWS_FM_MIN_BLOCK_LEN) return "block_len must be >= 20 (the reference's half-band keeps ten samples of a block)";
    if (nblocks < 0) return "nblocks must be >= 0";
    if (const char* why = ddc::why_not_cic_r(cic_r)) return why;
    if (const char* why = ddc::why_not_channels(nchannels)) return why;
    if (nblocks > LONG_MAX / ((long)block_len * 2 * cic_r)) return "nblocks * block_len too large";
    if (tiles_of(block_len, nblocks) + 1 > (long)INT_MAX / col_tiles(nchannels)) return "more tiles than one grid holds";
    return nullptr;
}

}  // namespace

extern "C" {

const char* rtlws_fmbank_last_error(void) { return g_err.c_str(); }

int rtlws_fmbank_supported(int cic_r, int nchannels, int block_len, long nblocks)
{
    return supported("rtlws_fmbank", why_not(cic_r, nchannels, block_len, nblocks));
}

int rtlws_fmbank_grid(int cic_r, int nchannels, int block_len, long nblocks, int* blocks, int* threads, int* lds_bytes,
                      int* tile_audio)
{
    g_err.clear();
    if (const char* why = why_not(cic_r, nchannels, block_len, nblocks)) return fail("rtlws_fmbank_grid", why, -1);
    const bool copy = nblocks == 0;                      // the state copy: one workgroup, no LDS
    if (blocks) *blocks = copy ? 1 : (int)((tiles_of(block_len, nblocks) + 1) * col_tiles(nchannels));
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = copy ? 0 : LDS_BYTES;
    if (tile_audio) *tile_audio = TILE;
    return 0;
}

rtlws_fmbank_plan* rtlws_fmbank_open(rtlws_engine* e)
{
    g_err.clear();
    return ddc::open_plan<rtlws_fmbank_plan>("rtlws_fmbank_open", nullptr, e, [](ddc::Plan&) { return prepare_bank(); });
}

void rtlws_fmbank_close(rtlws_fmbank_plan* p) { ddc::close_plan(p); }

int rtlws_fmbank_run(rtlws_fmbank_plan* p, int cic_r, const void* d_iq_cu8, int block_len, long nblocks,
                     long first_dec_index, int nchannels, const int* tuning_words, const float* d_state_in,
                     float* d_state_out, float* d_audio, long audio_stride, void* stream)
{
    const char* fn = "rtlws_fmbank_run";
    g_err.clear();
    if (const char* why = why_not(cic_r, nchannels, block_len, nblocks)) return fail(fn, why, -1);
    if (const char* why = ddc::why_not_first(first_dec_index)) return fail(fn, why, -1);
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

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    hipStream_t st = stream_of(p->engine, stream);
    if (nblocks == 0) {
        err = launch_state_copy(d_state_in, d_state_out, nchannels * STATE, st);
    } else {
        bp.src = d_iq_cu8;
        bp.table = p->d_table;
        bp.state_in = d_state_in;
        bp.state_out = d_state_out;
        bp.audio = d_audio;
        bp.audio_stride = audio_stride;
        bp.first = first_dec_index;
        bp.nblocks = nblocks;
        bp.ntiles = tiles_of(block_len, nblocks);
        bp.block_len = block_len;
        bp.cic_r = cic_r;
        bp.nch = nchannels;
        err = launch_bank(bp, st);
    }
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

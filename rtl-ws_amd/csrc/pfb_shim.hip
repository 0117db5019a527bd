// pfb_shim.hip -- extern "C" glue of include/rtlws_pfb.h (librtlws_pfb.so): the prototype design, the transform's
// table, argument rules, geometry, the launch.  The engine (device, stream) is librtlws_hip.so's; nothing here reads
// the environment, and nothing of a run is computed on the host: without a device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pfb_plan.h"
#include "rtlws_pfb.h"

struct rtlws_pfb_plan : rtlws::pfb::Plan {};

namespace {

using namespace rtlws::pfb;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && LAYOUT_CHANNEL == RTLWS_PFB_CHANNEL_MAJOR && LAYOUT_TIME == RTLWS_PFB_TIME_MAJOR,
              "rtlws_pfb.h and pfb_bank.h disagree");

// why a shape is not served, or nullptr; hop == 0: not asked
const char* why_not(int k, int taps, int hop, long nframes)
{
    if (const char* why = why_not_bank(k, taps)) return why;
    if (hop != 0)
        if (const char* why = why_not_hop(k, hop)) return why;
    return why_not_count(nframes, tile_frames(k), false);
}

}  // namespace

extern "C" {

const char* rtlws_pfb_last_error(void) { return g_err.c_str(); }

int rtlws_pfb_supported(int log2_channels, int taps_per_branch, int hop)
{
    return supported("rtlws_pfb", hop == 0 ? "hop must be M or M / 2" : why_not(log2_channels, taps_per_branch, hop, 0));
}

int rtlws_pfb_design(int log2_channels, int taps_per_branch, int16_t* taps)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, 0, 0)) return fail("rtlws_pfb_design", why, -1);
    if (!taps) return fail("rtlws_pfb_design", "null pointer", -1);
    const int M = 1 << log2_channels, N = taps_per_branch * M;
    for (int n = 0; n < N; ++n) {
        const double x = ((double)n - (double)(N - 1) / 2.0) / (double)M;
        const double sinc = x == 0.0 ? 1.0 : std::sin(M_PI * x) / (M_PI * x);
        const double w = 0.54 - 0.46 * std::cos(2.0 * M_PI * (double)n / (double)(N - 1));
        taps[n] = (int16_t)std::rint(32767.0 * sinc * w);
    }
    return 0;
}

int rtlws_pfb_twiddles(int log2_channels, float* re_im)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, 1, 0, 0)) return fail("rtlws_pfb_twiddles", why, -1);
    if (!re_im) return fail("rtlws_pfb_twiddles", "null pointer", -1);
    build_twiddles(log2_channels, re_im);
    return 0;
}

long rtlws_pfb_samples_needed(int log2_channels, int taps_per_branch, int hop, long nframes)
{
    g_err.clear();
    const char* why = hop == 0 ? "hop must be M or M / 2" : why_not(log2_channels, taps_per_branch, hop, nframes);
    if (why) return fail("rtlws_pfb_samples_needed", why, -1);
    if (nframes == 0) return 0;
    return (nframes - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfb_grid(int log2_channels, int taps_per_branch, int hop, long nframes, int* blocks, int* threads,
                   int* lds_bytes, int* tile_frames_out)
{
    g_err.clear();
    const char* why = hop == 0 ? "hop must be M or M / 2" : why_not(log2_channels, taps_per_branch, hop, nframes);
    if (why) return fail("rtlws_pfb_grid", why, -1);
    const int f = tile_frames(log2_channels);
    if (blocks) *blocks = (int)((nframes + f - 1) / f);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfb::lds_bytes(log2_channels);
    if (tile_frames_out) *tile_frames_out = f;
    return 0;
}

rtlws_pfb_plan* rtlws_pfb_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps)
{
    g_err.clear();
    return open_plan<rtlws_pfb_plan>("rtlws_pfb_open", why_not(log2_channels, taps_per_branch, 0, 0), e, log2_channels,
                                     taps_per_branch, taps, prepare_pfb);
}

void rtlws_pfb_close(rtlws_pfb_plan* p) { close_plan(p); }

int rtlws_pfb_run(rtlws_pfb_plan* p, const void* d_iq_cu8, long nframes, int hop, long first_frame_index, int layout,
                  void* d_out_cf32, long out_stride, void* stream)
{
    const char* fn = "rtlws_pfb_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a frame holds at least 16 values
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_count(nframes, tile_frames(MIN_LOG2_M), false)) return fail(fn, why, -1);
    if (first_frame_index < 0) return fail(fn, "first_frame_index must be >= 0", -1);
    if (layout != LAYOUT_CHANNEL && layout != LAYOUT_TIME) return fail(fn, "unknown layout", -1);
    if (out_stride < (layout == LAYOUT_CHANNEL ? nframes : 1L << MIN_LOG2_M)) return fail(fn, "out_stride too small for the layout", -1);
    if (nframes > 0 && (!d_iq_cu8 || !d_out_cf32)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u) return fail(fn, "d_iq_cu8 must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out_cf32) & 7u) return fail(fn, "d_out_cf32 must be 8-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan's shape decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, nframes)) return fail(fn, why, -1);
    if (layout == LAYOUT_TIME && out_stride < 1L << p->log2_m) return fail(fn, "out_stride too small for the layout", -1);
    if (nframes == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    PfbParams pp = bank_params(*p, hop, nframes);
    pp.src = d_iq_cu8;
    pp.out = static_cast<float2*>(d_out_cf32);
    pp.first = first_frame_index;
    pp.out_stride = out_stride;
    pp.layout = layout;
    err = launch_pfb(p->log2_m, pp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

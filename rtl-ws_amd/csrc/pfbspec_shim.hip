// pfbspec_shim.hip -- extern "C" glue of include/rtlws_pfbspec.h (librtlws_pfbspec.so): argument rules, geometry,
// the plan (pfb_plan.h's text, as librtlws_pfb.so's plan), the launch.  The engine (device, stream) is
// librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pfb_plan.h"
#include "pfbspec.h"
#include "rtlws_pfb.h"
#include "rtlws_pfbspec.h"

struct rtlws_pfbspec_plan : rtlws::pfb::Plan {};

namespace {

using namespace rtlws::pfb;
using namespace rtlws::pfbspec;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && MAX_K_AVG == RTLWS_PFBSPEC_MAX_K_AVG && OUT_SUM == RTLWS_OUT_POWER_SUM &&
                  OUT_DB == RTLWS_OUT_MEAN_DB && OUT_PAYLOAD == RTLWS_OUT_PAYLOAD_U8,
              "rtlws_pfbspec.h, rtlws_pfb.h, rtlws_hip.h and pfbspec.h disagree");

// why a run's shape is not served, or nullptr
const char* why_not(int k, int taps, int hop, int k_avg, long nspectra)
{
    if (const char* why = why_not_bank(k, taps)) return why;
    return why_not_sums(k, hop, k_avg, nspectra);
}

bool known_output(int output) { return output == OUT_SUM || output == OUT_DB || output == OUT_PAYLOAD; }

}  // namespace

extern "C" {

const char* rtlws_pfbspec_last_error(void) { return g_err.c_str(); }

int rtlws_pfbspec_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int output)
{
    const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, 0);
    if (!why && !known_output(output)) why = "unknown output";
    return supported("rtlws_pfbspec", why);
}

long rtlws_pfbspec_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, nspectra))
        return fail("rtlws_pfbspec_samples_needed", why, -1);
    if (nspectra == 0) return 0;
    return (nspectra * k_avg - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfbspec_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra, int* blocks, int* threads,
                       int* lds_bytes, int* spectra_per_block_out)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, nspectra))
        return fail("rtlws_pfbspec_grid", why, -1);
    const int g = spectra_per_block(log2_channels, k_avg);
    if (blocks) *blocks = (int)((nspectra + g - 1) / g);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfbspec::lds_bytes(log2_channels);
    if (spectra_per_block_out) *spectra_per_block_out = g;
    return 0;
}

rtlws_pfbspec_plan* rtlws_pfbspec_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps)
{
    g_err.clear();
    return open_plan<rtlws_pfbspec_plan>("rtlws_pfbspec_open", why_not_bank(log2_channels, taps_per_branch), e, log2_channels,
                                         taps_per_branch, taps, prepare_pfbspec);
}

void rtlws_pfbspec_close(rtlws_pfbspec_plan* p) { close_plan(p); }

int rtlws_pfbspec_run(rtlws_pfbspec_plan* p, const void* d_iq_cu8, long nspectra, int hop, int k_avg, int output, int shifted,
                      float scale, void* d_out, long out_stride, void* stream)
{
    const char* fn = "rtlws_pfbspec_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a row holds at least 16 values, a workgroup at most
    // 256 / k_avg spectra
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_k_avg(k_avg)) return fail(fn, why, -1);
    if (!known_output(output)) return fail(fn, "unknown output", -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (output != OUT_SUM && !(std::isfinite(scale) && scale > 0.0f)) return fail(fn, "scale must be finite and > 0", -1);
    if (const char* why = why_not_count(nspectra, spectra_per_block(MIN_LOG2_M, k_avg), true)) return fail(fn, why, -1);
    const int row_align = output == OUT_PAYLOAD ? 16 : 4;
    if (out_stride < 1L << MIN_LOG2_M) return fail(fn, "out_stride must be >= M", -1);
    if (out_stride % row_align) return fail(fn, output == OUT_PAYLOAD ? "out_stride must be a multiple of 16 for byte rows"
                                                                      : "out_stride must be a multiple of 4 for f32 rows", -1);
    if (nspectra > 0 && (!d_iq_cu8 || !d_out)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_iq_cu8) & 15u) return fail(fn, "d_iq_cu8 must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_out) & 15u) return fail(fn, "d_out must be 16-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan's shape decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, k_avg, nspectra)) return fail(fn, why, -1);
    if (out_stride < 1L << p->log2_m) return fail(fn, "out_stride must be >= M", -1);
    if (nspectra == 0) return 0;

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    SpecParams sp;
    sp.bank = bank_params(*p, hop, nspectra * k_avg);
    sp.bank.src = d_iq_cu8;
    sp.out = d_out;
    sp.nspectra = nspectra;
    sp.out_stride = out_stride;
    sp.k_avg = k_avg;
    sp.output = output;
    sp.shift = shifted ? 1 << (p->log2_m - 1) : 0;
    sp.lin = output == OUT_SUM ? 1.0f : scale / (float)k_avg;
    err = launch_pfbspec(p->log2_m, sp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"

// pfbxc_shim.hip -- extern "C" glue of include/rtlws_pfbxc.h (librtlws_pfbxc.so): argument rules, geometry, the plan
// (pfb_plan.h's text, as librtlws_pfb.so's and librtlws_pfbspec.so's plans), the launch.  The engine (device, stream)
// is librtlws_hip.so's; nothing here reads the environment, and nothing of a run is computed on the host: without a
// device there is no plan.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pfb_plan.h"
#include "pfbxc.h"
#include "rtlws_pfb.h"
#include "rtlws_pfbxc.h"

struct rtlws_pfbxc_plan : rtlws::pfb::Plan {
    int ninputs;
};

namespace {

using namespace rtlws::pfb;
using namespace rtlws::pfbxc;

static_assert(MIN_LOG2_M == RTLWS_PFB_MIN_LOG2_CHANNELS && MAX_LOG2_M == RTLWS_PFB_MAX_LOG2_CHANNELS &&
                  MAX_TAPS == RTLWS_PFB_MAX_TAPS && MAX_K_AVG == RTLWS_PFBXC_MAX_K_AVG && MIN_INPUTS == RTLWS_PFBXC_MIN_INPUTS &&
                  MAX_INPUTS == RTLWS_PFBXC_MAX_INPUTS,
              "rtlws_pfbxc.h, rtlws_pfb.h and pfbxc.h disagree");

// why a plan's shape is not served, or nullptr
const char* why_not_plan(int k, int taps, int ninputs)
{
    if (const char* why = why_not_bank(k, taps)) return why;
    if (ninputs < MIN_INPUTS || ninputs > MAX_INPUTS) return "ninputs must be 2 .. 4";
    return nullptr;
}

// why a run's shape is not served, or nullptr
const char* why_not(int k, int taps, int hop, int k_avg, int ninputs, long nspectra)
{
    if (const char* why = why_not_plan(k, taps, ninputs)) return why;
    return why_not_sums(k, hop, k_avg, nspectra);
}

}  // namespace

extern "C" {

const char* rtlws_pfbxc_last_error(void) { return g_err.c_str(); }

int rtlws_pfbxc_supported(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs)
{
    return supported("rtlws_pfbxc", why_not(log2_channels, taps_per_branch, hop, k_avg, ninputs, 0));
}

long rtlws_pfbxc_samples_needed(int log2_channels, int taps_per_branch, int hop, int k_avg, long nspectra)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, MIN_INPUTS, nspectra))
        return fail("rtlws_pfbxc_samples_needed", why, -1);
    if (nspectra == 0) return 0;
    return (nspectra * k_avg - 1) * hop + (long)taps_per_branch * (1L << log2_channels);
}

int rtlws_pfbxc_pair_index(int ninputs, int a, int b)
{
    if (ninputs < MIN_INPUTS || ninputs > MAX_INPUTS || a < 0 || a >= b || b >= ninputs) return -1;
    // the pairs (a', b') with a' < a come first: sum_{a' < a} (ninputs - 1 - a')
    return a * (2 * ninputs - a - 1) / 2 + (b - a - 1);
}

int rtlws_pfbxc_grid(int log2_channels, int taps_per_branch, int hop, int k_avg, int ninputs, long nspectra, int* blocks,
                     int* threads, int* lds_bytes, int* spectra_per_block_out)
{
    g_err.clear();
    if (const char* why = why_not(log2_channels, taps_per_branch, hop, k_avg, ninputs, nspectra))
        return fail("rtlws_pfbxc_grid", why, -1);
    const int g = spectra_per_block(log2_channels, k_avg);
    if (blocks) *blocks = (int)((nspectra + g - 1) / g);
    if (threads) *threads = THREADS;
    if (lds_bytes) *lds_bytes = rtlws::pfbxc::lds_bytes(log2_channels, ninputs);
    if (spectra_per_block_out) *spectra_per_block_out = g;
    return 0;
}

rtlws_pfbxc_plan* rtlws_pfbxc_open(rtlws_engine* e, int log2_channels, int taps_per_branch, const int16_t* taps, int ninputs)
{
    g_err.clear();
    rtlws_pfbxc_plan* p = open_plan<rtlws_pfbxc_plan>("rtlws_pfbxc_open", why_not_plan(log2_channels, taps_per_branch, ninputs), e,
                                                      log2_channels, taps_per_branch, taps,
                                                      [ninputs](int k) { return prepare_pfbxc(k, ninputs); });
    if (p) p->ninputs = ninputs;
    return p;
}

void rtlws_pfbxc_close(rtlws_pfbxc_plan* p) { close_plan(p); }

int rtlws_pfbxc_run(rtlws_pfbxc_plan* p, const void* const* d_iq_cu8, long nspectra, int hop, int k_avg, int shifted,
                    float* d_auto, long auto_stride, float* d_cross, long cross_stride, void* stream)
{
    const char* fn = "rtlws_pfbxc_run";
    g_err.clear();
    // what needs no plan: the hop is a power of two 8 .. 1024, a row holds at least 16 values, a workgroup at most
    // 256 / k_avg spectra
    if (const char* why = why_not_any_hop(hop)) return fail(fn, why, -1);
    if (const char* why = why_not_k_avg(k_avg)) return fail(fn, why, -1);
    if (shifted != 0 && shifted != 1) return fail(fn, "shifted must be 0 or 1", -1);
    if (const char* why = why_not_count(nspectra, spectra_per_block(MIN_LOG2_M, k_avg), true)) return fail(fn, why, -1);
    if (auto_stride < 1L << MIN_LOG2_M) return fail(fn, "auto_stride must be >= M", -1);
    if (auto_stride % 4) return fail(fn, "auto_stride must be a multiple of 4", -1);
    if (cross_stride < 1L << MIN_LOG2_M) return fail(fn, "cross_stride must be >= M", -1);
    if (cross_stride % 2) return fail(fn, "cross_stride must be a multiple of 2", -1);
    if (nspectra > 0 && (!d_iq_cu8 || !d_auto || !d_cross)) return fail(fn, "null pointer", -1);
    if (reinterpret_cast<uintptr_t>(d_auto) & 15u) return fail(fn, "d_auto must be 16-byte aligned", -1);
    if (reinterpret_cast<uintptr_t>(d_cross) & 15u) return fail(fn, "d_cross must be 16-byte aligned", -1);
    if (!p) return fail(fn, "null plan (no usable HIP device: there is no CPU path)", -1);
    // what the plan decides; still before anything is asked of the device
    if (const char* why = why_not(p->log2_m, p->taps_per_branch, hop, k_avg, p->ninputs, nspectra)) return fail(fn, why, -1);
    if (auto_stride < 1L << p->log2_m) return fail(fn, "auto_stride must be >= M", -1);
    if (cross_stride < 1L << p->log2_m) return fail(fn, "cross_stride must be >= M", -1);
    if (nspectra == 0) return 0;
    if (const char* why = why_not_captures(d_iq_cu8, p->ninputs)) return fail(fn, why, -1);

    hipError_t err = hipSetDevice(p->device);
    if (err != hipSuccess) return fail_hip(fn, "hipSetDevice", err);
    XcParams xp;
    xp.bank = bank_params(*p, hop, nspectra * k_avg);
    for (int a = 0; a < MAX_INPUTS; ++a) xp.src[a] = a < p->ninputs ? d_iq_cu8[a] : nullptr;
    xp.autos = d_auto;
    xp.cross = reinterpret_cast<float2*>(d_cross);
    xp.nspectra = nspectra;
    xp.auto_stride = auto_stride;
    xp.cross_stride = cross_stride;
    xp.k_avg = k_avg;
    xp.shift = shifted ? 1 << (p->log2_m - 1) : 0;
    err = launch_pfbxc(p->log2_m, p->ninputs, xp, stream_of(p->engine, stream));
    if (err != hipSuccess) return fail_hip(fn, "kernel launch", err);
    return 0;
}

}  // extern "C"
